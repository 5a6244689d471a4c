"""Frame-level models on [B, F<=300, D] + num_frames; class names, flags and TF variable names mirror
W/frame_level_models.py + W/all_frame_models/ (W = /root/reference/youtube-8m-wangheda).
NetVLADModel / GatedNetVLADModel are NOT in the reference; they follow SURVEY.md Appendix B.
"""
import math

import torch

from . import models, model_utils, ops, seq_ops, video_level_models
from .video_level_models import (composed_link, distill_link as _distill_link, fused_link, moe_stage, prediction_chain, relu_kind,
                                 relu_link)
from .flags import FLAGS, DEFINE_integer, DEFINE_bool, DEFINE_string
from .variables import constant, get_default_graph, glorot_uniform, ones, random_normal, truncated_normal, xavier_uniform, zeros

# W/frame_level_models.py:20-84 (hot-path subset)
DEFINE_integer("iterations", 30, "Number of frames per batch for DBoF.")
DEFINE_bool("dbof_add_batch_norm", True, "Adds batch normalization to the DBoF model.")
DEFINE_bool("sample_random_frames", True, "If true samples random frames (for frame level models). If false, a random"
            "sequence of frames is sampled instead.")
DEFINE_integer("dbof_cluster_size", 8192, "Number of units in the DBoF cluster layer.")
DEFINE_integer("dbof_hidden_size", 1024, "Number of units in the DBoF hidden layer.")
DEFINE_string("dbof_pooling_method", "max", "The pooling method used in the DBoF cluster layer. Choices are 'average' and 'max'.")
DEFINE_string("video_level_classifier_model", "MoeModel", "Some Frame-Level models can be decomposed into a "
              "generalized pooling operation followed by a classifier layer")
DEFINE_bool("rnn_swap_memory", False, "If true, swap_memory = True.  (No numerical effect; ignored: 288 GB HBM.)")
DEFINE_string("lstm_cells", "1024", "Number of LSTM cells.")
DEFINE_integer("lstm_layers", 2, "Number of LSTM layers.")
# new: time chunks of the layer-pipelined LSTM stack (1 = one layer after the other)
DEFINE_integer("gru_cells", 1024, "Number of GRU cells.")
DEFINE_integer("gru_layers", 2, "Number of GRU layers.")
DEFINE_integer("lstm_pipeline_chunks", 2, "Time chunks over which the layers of the LSTM stack are pipelined on separate streams.")
DEFINE_string("feature_sizes", "1024", "Length of the feature vectors.")     # W/train.py:58 (read by the parallel LSTM model)
DEFINE_integer("positional_embedding_size", 32, "Positional embedding dimension use in lstm_positional_attention_max_pooling_model.")
DEFINE_integer("lstm_attentions", 8, "Attention size in lstm_attention_max_pooling_model.")
DEFINE_integer("attention_size", 1, "Number of attention layers.")                                   # W/frame_level_models.py:49
DEFINE_bool("is_training", False, "used in batch normalization.")
DEFINE_integer("multiscale_cnn_lstm_layers", 1, "number of layers in multiscale cnn_lstm.")          # W/frame_level_models.py:77
DEFINE_integer("distillchain_relu_cells", 256, "number of relu cells in distillchain model.")        # W/frame_level_models.py:81
DEFINE_integer("deep_cnn_base_size", 128, "Base number of cnn filters in deep cnn models.")          # W/frame_level_models.py:65
# new (Appendix B)
DEFINE_integer("netvlad_cluster_size", 64, "Number of NetVLAD clusters.")
DEFINE_integer("netvlad_hidden_size", 1024, "Width of the FC after the VLAD descriptor.")
DEFINE_bool("netvlad_gating", False, "Context gating after the hidden FC.")
DEFINE_bool("netvlad_add_batch_norm", False, "Kept False so examples stay independent under data parallelism.")


def _head(name=None):
    return getattr(video_level_models, name or FLAGS.video_level_classifier_model)


def _classify(head_input, model_input, vocab_size, **params):
    """The video-level classifier (--video_level_classifier_model) on head_input; params: what the calling plugin forwards to it."""
    return _head()().create_model(model_input=head_input, original_input=model_input, vocab_size=vocab_size, **params)


def _sizes_per_feature():
    """(--lstm_cells, --feature_sizes) as lists of ints: one LSTM size per input feature."""
    lstm_sizes, feature_sizes = ([int(v) for v in str(flag).split(",")] for flag in (FLAGS.lstm_cells, FLAGS.feature_sizes))
    assert len(lstm_sizes) == len(feature_sizes), \
        "length of lstm_sizes (={}) != length of feature_sizes (={})".format(len(lstm_sizes), len(feature_sizes))
    return lstm_sizes, feature_sizes


def _lib_u8_ok(D):
    from . import _lib
    return bool(_lib.lib().yt8m_u8_proj_supported(int(D)))


def _bytes_or_floats(model_input, num_frames, supported):
    """(input, is_bytes): the reader's bytes [B,F,D] where supported(q) says that the calling plugin's byte kernels cover the shape, else
    the dequantised, l2-normalised float frames the reference's transformer would have handed over (float input passes through)."""
    if model_input.dtype != torch.uint8:
        return model_input, False
    if supported(model_input):
        return model_input.contiguous(), True
    return ops.dequant_l2norm(model_input, num_frames), False


def _mean_frame(x, num_frames, rs=None, clamp=False):
    """sum_f x[b, f] / num_frames [B,D] over the video's frames; clamp: / max(num_frames, 1), and all F frames without num_frames.
    Bytes: one weighted pooling pass over them (rs = seq_ops.u8_frame_scales, 0 on the padding frames; made here unless the plugin has it
    already).  Floats: masked sum.  The frames are data: no gradient flows here."""
    B, F, D = x.shape
    n = None if num_frames is None else num_frames.to(torch.float32)
    if clamp and n is not None:
        n = n.clamp(min=1)
    if x.dtype == torch.uint8:
        if rs is None:
            rs = seq_ops.u8_frame_scales(x, num_frames)
        inv = torch.full((B,), 1.0 / F, dtype=torch.float32, device=x.device) if n is None else 1.0 / n
        return seq_ops.pool_u8_raw(inv.view(B, 1, 1).expand(B, F, 1).contiguous(), x, rs).view(B, D)
    if n is None:
        return x.sum(dim=1) / float(F)
    mask = (torch.arange(F, device=x.device)[None, :] < num_frames[:, None]).to(x.dtype)
    return (x * mask[:, :, None]).sum(dim=1) / n.to(x.dtype)[:, None]


def _stack_input(model_input, num_frames, dropping=False):
    """What the native stack reads: the raw reader bytes [B,F,D] where its layer-0 projection consumes them directly (csrc/u8proj.hip:
    exact bf16 operands, the dequantise / l2-normalise affine folded into the GEMM epilogue -- no fp32 [B,F,D] tensor, no transpose
    copy; not under a DropoutWrapper), else float frames time-major [F,B,D] (dequantised first when they arrive as bytes)."""
    x, u8 = _bytes_or_floats(model_input, num_frames, lambda q: _lib_u8_ok(q.shape[2]) and not dropping)
    return x if u8 else x.transpose(0, 1).contiguous()          # bytes: re-ordered time-major by the conversion pass; floats: layout glue


def _native_stack(x_tm, num_frames, wb, **kwargs):
    """seq_ops.lstm_stack as every plugin here runs it: BasicLSTMCell(forget_bias=1.0), the flags' pipeline chunks and compute dtype."""
    return seq_ops.lstm_stack(x_tm, num_frames, wb, forget_bias=1.0, chunks=FLAGS.lstm_pipeline_chunks,
                              bf16=FLAGS.compute_dtype == "bfloat16", **kwargs)


def _lstm_cells(d_in, lstm_size, number_of_layers, multi=True):
    """BasicLSTMCell variables in the current scope: multi_rnn_cell/cell_<l>/basic_lstm_cell/{weights,biases} for a MultiRNNCell,
    basic_lstm_cell/{weights,biases} for a lone cell.  Returns [(W_l, b_l)]."""
    g = get_default_graph()
    wb = []
    for l in range(number_of_layers):
        scope = "multi_rnn_cell/cell_%d/basic_lstm_cell" % l if multi else "basic_lstm_cell"
        W = g.get_variable(scope + "/weights", (d_in + lstm_size, 4 * lstm_size), xavier_uniform)
        b = g.get_variable(scope + "/biases", (4 * lstm_size,), zeros)
        wb.append((W, b))
        d_in = lstm_size
    return wb


def _lstm_stack(model_input, num_frames, lstm_size, number_of_layers, scope="RNN", input_keep_prob=None, **kwargs):
    """MultiRNNCell([BasicLSTMCell(H, forget_bias=1.0)] * L) under tf.nn.dynamic_rnn inside variable_scope("RNN")
    (W/all_frame_models/lstm_model.py:34-47).  TF-1.0 variable names:
    RNN/multi_rnn_cell/cell_<l>/basic_lstm_cell/{weights,biases}.  Returns time-major outputs of the top layer
    and the per-layer final (c, h)."""
    g = get_default_graph()
    dropping = input_keep_prob is not None and float(input_keep_prob) < 1.0
    x_tm = _stack_input(model_input, num_frames, dropping)
    with g.variable_scope(scope):
        wb = _lstm_cells(model_input.shape[2], lstm_size, number_of_layers)
    # all layers in one op: layer l+1 works on time chunk c while layer l is already in chunk c+1 (seq_ops._LstmStack)
    return _native_stack(x_tm, num_frames, wb, input_keep_prob=input_keep_prob, **kwargs)


class FrameLevelLogisticModel(models.BaseModel):
    """W/all_frame_models/logistic_model.py:13-46: logistic classifier over the num_frames-average of the frames."""

    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        model_input, u8 = _bytes_or_floats(model_input, num_frames, lambda q: seq_ops.u8_attention_supported(q, 1))
        if u8:
            avg_pooled = _mean_frame(model_input, num_frames)
        else:
            denominators = num_frames.to(torch.float32).unsqueeze(1)
            avg_pooled = model_input.sum(dim=1) / denominators     # input is data: no gradient flows here
        output = video_level_models.fully_connected(avg_pooled, vocab_size, "fully_connected", activation="sigmoid",
                                                    l2_penalty=1e-8)
        return {"predictions": output}


class LstmModel(models.BaseModel):
    """W/all_frame_models/lstm_model.py:13-57: the head reads the whole final state [c0||h0||c1||h1]
    (state_is_tuple=False), 4H wide for two layers.  accepts_quantized_input: see _lstm_stack."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        lstm_size = int(FLAGS.lstm_cells)
        number_of_layers = FLAGS.lstm_layers
        _, finals = _lstm_stack(model_input, num_frames, lstm_size, number_of_layers)
        state = torch.cat([t for pair in finals for t in pair], dim=1)
        return _classify(state, model_input, vocab_size, **unused_params)


def _bidirectional_stacks(model_input, num_frames, lstm_size, number_of_layers, multi):
    """tf.nn.bidirectional_dynamic_rnn(cell_fw, cell_bw, x, sequence_length=num_frames) inside variable_scope("RNN") (TF 1.0: the
    directions live in bidirectional_rnn/fw and bidirectional_rnn/bw).  The bw direction is the ordinary stack on
    reverse_sequence(x, num_frames): on the byte path the reader's bytes are reversed (csrc/sequence.hip) and go to the stack's byte
    product as they are, else the float frames are reversed time-major.  Its final state is the state after original frame 0; its
    outputs come back in REVERSED time (callers that need them in frame order reverse them again: seq_ops.bi_concat).
    Returns ((out_fw, finals_fw), (out_bw_reversed, finals_bw))."""
    g = get_default_graph()
    x_fw = _stack_input(model_input, num_frames)
    x_bw = seq_ops.reverse_sequence_u8(x_fw, num_frames) if x_fw.dtype == torch.uint8 else seq_ops.reverse_sequence_tm(x_fw, num_frames)
    d_in = model_input.shape[2]
    with g.variable_scope("RNN"):
        with g.variable_scope("bidirectional_rnn"):
            with g.variable_scope("fw"):
                wb_fw = _lstm_cells(d_in, lstm_size, number_of_layers, multi)
            with g.variable_scope("bw"):
                wb_bw = _lstm_cells(d_in, lstm_size, number_of_layers, multi)
    return seq_ops.bidirectional_lstm_stacks(x_fw, x_bw, num_frames, wb_fw, wb_bw, forget_bias=1.0, chunks=FLAGS.lstm_pipeline_chunks,
                                             bf16=FLAGS.compute_dtype == "bfloat16")


class BiLstmModel(models.BaseModel):
    """W/all_frame_models/bilstm_model.py:13-60: MultiRNNCell([BasicLSTMCell(H)] * L, state_is_tuple=False) per direction under
    tf.nn.bidirectional_dynamic_rnn in variable_scope("RNN"); the head reads [state_fw || state_bw], each [c0||h0||c1||h1...]
    (2 L 2H wide).  Variable names as TF 1.0 builds them, written from memory (as SURVEY.md Appendix A):
    RNN/bidirectional_rnn/{fw,bw}/multi_rnn_cell/cell_<l>/basic_lstm_cell/{weights,biases} (pinned in tests/test_bilstm_host.py).
    accepts_quantized_input: both directions' stacks read the reader's bytes (the bw one reversed per video)."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        lstm_size = int(FLAGS.lstm_cells)
        (_, fin_fw), (_, fin_bw) = _bidirectional_stacks(model_input, num_frames, lstm_size, FLAGS.lstm_layers, multi=True)
        state = torch.cat([t for pair in fin_fw + fin_bw for t in pair], dim=1)
        return _classify(state, model_input, vocab_size, **unused_params)


class BiUniLstmModel(models.BaseModel):
    """W/all_frame_models/biunilstm_model.py:13-60: one BasicLSTMCell(H) per direction under tf.nn.bidirectional_dynamic_rnn, their
    outputs concatenated ([B,F,2H]: out_fw || reverse_sequence(out_bw)), a third BasicLSTMCell(H) over that (dynamic_rnn with the
    same sequence_length); the head reads [c_fw||h_fw||c_bw||h_bw||c_2||h_2] (6H).  Variable names (TF 1.0, from memory):
    RNN/bidirectional_rnn/{fw,bw}/basic_lstm_cell/{weights,biases} and, for the third cell -- a dynamic_rnn without a scope argument,
    which this project maps to no extra scope (as for LstmModel) -- RNN/basic_lstm_cell/{weights,biases}."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        lstm_size = int(FLAGS.lstm_cells)
        (out_fw, fin_fw), (out_bw, fin_bw) = _bidirectional_stacks(model_input, num_frames, lstm_size, 1, multi=False)
        l1 = seq_ops.bi_concat(out_fw, out_bw, num_frames)          # [F,B,2H] time-major, bw half back in frame order
        g = get_default_graph()
        with g.variable_scope("RNN"):
            wb2 = _lstm_cells(2 * lstm_size, lstm_size, 1, multi=False)
        _, fin2 = _native_stack(l1, num_frames, wb2, slot=2)
        state = torch.cat([t for pair in fin_fw + fin_bw + fin2 for t in pair], dim=1)
        return _classify(state, model_input, vocab_size, **unused_params)


class LstmMemoryModel(models.BaseModel):
    """W/all_frame_models/lstm_memory_model.py:13-73: the head reads the concatenated c states (2H)."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, dropout=False, keep_prob=None, noise_level=None,
                     **unused_params):
        lstm_size = int(FLAGS.lstm_cells)
        number_of_layers = FLAGS.lstm_layers
        # :36-45 DropoutWrapper(BasicLSTMCell, input_keep_prob=keep_prob) around every layer when --dropout
        _, finals = _lstm_stack(model_input, num_frames, lstm_size, number_of_layers,
                                input_keep_prob=keep_prob if dropout else None)
        final_state = torch.cat([c for c, _ in finals], dim=1)
        if noise_level is not None:
            final_state = ops.add_noise(final_state, noise_level)
        return _classify(final_state, model_input, vocab_size, num_frames=num_frames, **unused_params)


def _hoisted_input(model_input, num_frames):
    """Layer-0 input of a GRU / LayerNorm-LSTM stack: the reader's bytes as operand images (seq_ops.U8FrameImages: the hoisted input
    projection and its weight gradient read them, no fp32 [B,F,D] tensor) where the byte products cover the shape, else the float
    frames time-major [F,B,D] (dequantised first when they arrive as bytes)."""
    x, u8 = _bytes_or_floats(model_input, num_frames, seq_ops.u8_hoisted_supported)
    return seq_ops.U8FrameImages(x, num_frames) if u8 else x.transpose(0, 1).contiguous()          # (layout glue)


def _gru_stack(model_input, num_frames, gru_size, number_of_layers):
    """MultiRNNCell([GRUCell(H)] * L, state_is_tuple=False) under tf.nn.dynamic_rnn in variable_scope("RNN")
    (W/all_frame_models/gru_pooling_model.py:34-47).  TF-1.0 names: RNN/multi_rnn_cell/cell_<l>/gru_cell/{gates,candidate}/
    {weights,biases}; the gate bias starts at 1.  Returns (top outputs time-major [F,B,H], [h_l final])."""
    g = get_default_graph()
    x_tm = _hoisted_input(model_input, num_frames)
    finals = []
    d_in = model_input.shape[2]
    with g.variable_scope("RNN"):
        for l in range(number_of_layers):
            scope = "multi_rnn_cell/cell_%d/gru_cell" % l
            Wg = g.get_variable(scope + "/gates/weights", (d_in + gru_size, 2 * gru_size), xavier_uniform)
            bg = g.get_variable(scope + "/gates/biases", (2 * gru_size,), ones)
            Wc = g.get_variable(scope + "/candidate/weights", (d_in + gru_size, gru_size), xavier_uniform)
            bc = g.get_variable(scope + "/candidate/biases", (gru_size,), zeros)
            x_tm, h = seq_ops.gru_layer(x_tm, Wg, bg, Wc, bc, num_frames)
            finals.append(h)
            d_in = gru_size
    return x_tm, finals


def _mean_over_frames(out_tm, num_frames):
    """reduce_sum(outputs, axis=1) / max(num_frames, 1) (W/all_frame_models/gru_pooling_model.py:48-49): dynamic_rnn outputs
    are zero past num_frames, so this is one [1,F] x [F,H] product per video with constant weights 1 / max(num_frames, 1)."""
    F, B, H = out_tm.shape
    w = (1.0 / num_frames.to(torch.float32).clamp(min=1.0)).view(B, 1, 1).expand(B, F, 1).contiguous()
    return seq_ops.pool_tn(w, out_tm.transpose(0, 1).contiguous()).view(B, H)


class GruPoolingModel(models.BaseModel):
    """W/all_frame_models/gru_pooling_model.py:13-58: GRU stack, head input = outputs averaged over the video's frames.
    (The reference file divides by tf.maximum(num_frames, tf.ones([batch_size, 1])) with `batch_size` undefined -- it raises
    NameError at graph construction; built here with the evident meaning.)"""
    accepts_quantized_input = True                         # _hoisted_input: layer 0 reads the reader's bytes

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        out_tm, _ = _gru_stack(model_input, num_frames, FLAGS.gru_cells, FLAGS.gru_layers)
        pooling_output = _mean_over_frames(out_tm, num_frames)
        return _classify(pooling_output, model_input, vocab_size, **unused_params)


class GruWithPoolingModel(models.BaseModel):
    """W/all_frame_models/gru_with_pooling_model.py:13-60: head input = [mean-pooled outputs || final state of every layer]
    (state_is_tuple=False: [h_0 || h_1 ...]).  Same `batch_size` NameError in the reference as GruPoolingModel."""
    accepts_quantized_input = True                         # _hoisted_input: layer 0 reads the reader's bytes

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        out_tm, finals = _gru_stack(model_input, num_frames, FLAGS.gru_cells, FLAGS.gru_layers)
        final_output = torch.cat([_mean_over_frames(out_tm, num_frames)] + finals, dim=1)
        return _classify(final_output, model_input, vocab_size, **unused_params)


LN_GATES = ("input", "transform", "forget", "output", "state")


class LayerNormLstmMemoryModel(models.BaseModel):
    """W/all_frame_models/layernorm_lstm_memory_model.py:13-72: MultiRNNCell([LayerNormBasicLSTMCell(H)] * L); with --dropout the
    cells get dropout_keep_prob=keep_prob (recurrent dropout on the candidate); head input = concat of the (normalised) c
    states.  TF-1.0 names: RNN/multi_rnn_cell/cell_<l>/layer_norm_basic_lstm_cell/{weights, <gate>/gamma, <gate>/beta}."""
    accepts_quantized_input = True                         # _hoisted_input: layer 0 reads the reader's bytes

    def create_model(self, model_input, vocab_size, num_frames, dropout=False, keep_prob=None, noise_level=None,
                     **unused_params):
        lstm_size = int(FLAGS.lstm_cells)
        g = get_default_graph()
        x_tm = _hoisted_input(model_input, num_frames)
        cs = []
        d_in = model_input.shape[2]
        with g.variable_scope("RNN"):
            for l in range(FLAGS.lstm_layers):
                scope = "multi_rnn_cell/cell_%d/layer_norm_basic_lstm_cell" % l
                W = g.get_variable(scope + "/weights", (d_in + lstm_size, 4 * lstm_size), xavier_uniform)
                gammas = [g.get_variable("%s/%s/gamma" % (scope, n), (lstm_size,), ones) for n in LN_GATES]
                betas = [g.get_variable("%s/%s/beta" % (scope, n), (lstm_size,), zeros) for n in LN_GATES]
                x_tm, c, _ = seq_ops.lnlstm_layer(x_tm, W, gammas, betas, num_frames, forget_bias=1.0,
                                                  keep_prob=keep_prob if (dropout and keep_prob is not None) else 1.0)
                cs.append(c)
                d_in = lstm_size
        final_state = torch.cat(cs, dim=1)
        if noise_level is not None:
            final_state = ops.add_noise(final_state, noise_level)
        return _classify(final_state, model_input, vocab_size, **unused_params)


def _attention_fc_u8(q, num_frames, parts, num_outputs, scope, l2_penalty, rs=None):
    """slim.fully_connected(concat([x] + parts)) with x = the raw frames (same variables as video_level_models.fully_connected_cat);
    parts: [B,F,K] per-frame tensors and [B,K] per-video vectors (tiled over the frames by the reference), in concatenation order."""
    g = get_default_graph()
    width = q.shape[2] + sum(p.shape[-1] for p in parts)
    W = g.get_variable(scope + "/weights", (width, num_outputs), xavier_uniform, l2=l2_penalty)
    b = g.get_variable(scope + "/biases", (num_outputs,), zeros)
    if rs is None:
        rs = seq_ops.u8_frame_scales(q, num_frames)                                 # [B,F]; 0 on the padding frames
    return seq_ops.attention_logits_u8(q, rs, None, W, b, parts=parts)


class LstmAttentionMaxPoolingModel(models.BaseModel):
    """W/all_frame_models/lstm_attention_max_pooling_model.py:10-98: LSTM outputs -> A attention poolings ->
    MoE per attention -> max over attentions.  accepts_quantized_input: the stack (see _lstm_stack) and the attention FC read the raw
    reader bytes; no fp32 [B,F,D] tensor."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, num_mixtures=None, l2_penalty=1e-8, sub_scope="",
                     original_input=None, **unused_params):
        lstm_size = int(FLAGS.lstm_cells)
        number_of_layers = FLAGS.lstm_layers
        num_attentions = FLAGS.lstm_attentions
        # bytes: raw reader bytes into the stack AND the attention FC
        model_input, u8 = _bytes_or_floats(model_input, num_frames, lambda q: _lib_u8_ok(q.shape[2]) and
                                           seq_ops.u8_attention_supported(q, num_attentions))
        out_tm, _ = _lstm_stack(model_input, num_frames, lstm_size, number_of_layers)
        outputs = out_tm.transpose(0, 1).contiguous()                               # [B,F,H]
        parts, rs = self.attention_parts(model_input, num_frames, l2_penalty)
        if u8:
            attention_activations = _attention_fc_u8(model_input, num_frames, parts + [outputs], num_attentions, "attention-" + sub_scope,
                                                     l2_penalty, rs=rs)
        else:
            attention_activations = video_level_models.fully_connected_cat(           # :51-56 FC on concat([input, ..., outputs])
                [model_input] + parts + [outputs], num_attentions, "attention-" + sub_scope, l2_penalty=l2_penalty)
        attention_weights = seq_ops.attention_weights(attention_activations, num_frames)   # [B,F,A]
        attention_outputs = seq_ops.pool_tn(attention_weights, outputs)                    # [B,A,H]
        moe_predictions = self.sub_moe(self._moe_input(attention_outputs), vocab_size, sub_scope="sub-moe")
        predictions = moe_predictions.view(-1, num_attentions, vocab_size)
        max_predictions = ops.frame_pool(predictions, "max")          # tf.reduce_max over the attentions
        return {"predictions": max_predictions}

    def attention_parts(self, model_input, num_frames, l2_penalty):
        """(what the attention FC sees between the frames and the LSTM outputs, the bytes' frame scales if they were needed): nothing."""
        return [], None

    def _moe_input(self, attention_outputs):
        """What sub_moe reads, from the attention outputs [B,A,H]: the attention outputs."""
        return attention_outputs

    def sub_moe(self, model_input, vocab_size, **params):
        return moe_stage(model_input, vocab_size, **params)


def _sigmoid_attention_fc(src_tm, num_frames, attention_size, scope, l2_penalty, values_tm=None):
    """slim.fully_connected(outputs, attention_size, activation_fn=tf.nn.sigmoid, weights_regularizer=l2) under `scope`, masked by
    num_frames and divided by its sum over the frames plus 1e-8 (W/all_frame_models/lstm_attention_model.py:61-71), on the time-major
    outputs src_tm [F,B,H] of a stack.  Returns (attention [B,F,A], sum_t attention * values_tm [B,A,Hv] or None): seq_ops.sigmoid_attention."""
    g = get_default_graph()
    W = g.get_variable(scope + "/weights", (src_tm.shape[2], attention_size), xavier_uniform, l2=l2_penalty)
    b = g.get_variable(scope + "/biases", (attention_size,), zeros)
    return seq_ops.sigmoid_attention(src_tm, W, b, num_frames, values_tm)


def _attend_frames(attention, model_input, num_frames):
    """sum_t attention[b,t,a] * model_input[b,t,:] [B,A,D]: on the reader's bytes one weighted pooling pass over them (no fp32 copy of
    the frames), on float frames pool_tn.  The frames are data: the gradient goes to the attention only."""
    if model_input.dtype == torch.uint8:
        return seq_ops.pool_tn_u8(attention, model_input, seq_ops.u8_frame_scales(model_input, num_frames))
    return seq_ops.pool_tn(attention, model_input)


class LstmAttentionModel(models.BaseModel):
    """W/all_frame_models/lstm_attention_model.py:13-83: an LSTM stack under RNN; one sigmoid per frame from a fully connected layer on
    its top outputs, masked and normalised over the video's frames, weighs the INPUT frames; the head reads [mean_input | state], state
    in LstmModel's state_is_tuple=False order [c0|h0|c1|h1...].  Variables (TF 1.0, from memory): RNN/multi_rnn_cell/cell_<l>/
    basic_lstm_cell/{weights,biases} and RNN/fully_connected/{weights,biases} (the FC sits inside the RNN scope; its weights carry
    l2_penalty).  The reference's mask_emb, a non-trainable [F+1,F] lookup table of frame masks, is left out: the mask is computed
    from num_frames.  accepts_quantized_input: the stack (see _lstm_stack) and the pooling read the reader's bytes."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        lstm_size = int(FLAGS.lstm_cells)
        l2_penalty = unused_params.get("l2_penalty", 1e-8)
        model_input, _ = _bytes_or_floats(model_input, num_frames, lambda q: _lib_u8_ok(q.shape[2]) and seq_ops.u8_attention_supported(q, 1))
        out_tm, finals = _lstm_stack(model_input, num_frames, lstm_size, FLAGS.lstm_layers)
        attention, _ = _sigmoid_attention_fc(out_tm, num_frames, 1, "RNN/fully_connected", l2_penalty)
        mean_input = _attend_frames(attention, model_input, num_frames).view(model_input.shape[0], model_input.shape[2])
        state = torch.cat([t for pair in finals for t in pair], dim=1)
        return _classify(torch.cat([mean_input, state], dim=1), model_input, vocab_size, **unused_params)


class LstmAttentionLstmModel(models.BaseModel):
    """W/all_frame_models/lstm_attention_lstm_model.py:13-102: two LSTM stacks over the same input, ATT and RNN; the sigmoid attention
    comes from the ATT stack's top outputs and weighs the RNN stack's top outputs; the head reads [attended_output | ATT final memories
    c | RNN final memories c].  Variables (TF 1.0, from memory): {ATT,RNN}/multi_rnn_cell/cell_<l>/basic_lstm_cell/{weights,biases} and
    RNN/fully_connected/{weights,biases} (l2_penalty on the weights).  mask_emb is left out as in LstmAttentionModel.
    accepts_quantized_input: both stacks read the reader's bytes (see _lstm_stack); logit, gate, mask, sums and the pooling of the RNN
    outputs are one pass over the two time-major output tensors (seq_ops.sigmoid_attention)."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        lstm_size = int(FLAGS.lstm_cells)
        number_of_layers = FLAGS.lstm_layers
        l2_penalty = unused_params.get("l2_penalty", 1e-8)
        g = get_default_graph()
        x_tm = _stack_input(model_input, num_frames)                 # prepared once, read by both stacks
        seq_ops.reserve_resident(2, number_of_layers)
        stacks = []
        for slot, scope in enumerate(("ATT", "RNN")):                # both stacks' outputs are alive together: slots of their own
            with g.variable_scope(scope):
                wb = _lstm_cells(model_input.shape[2], lstm_size, number_of_layers)
            stacks.append(_native_stack(x_tm, num_frames, wb, slot=slot))
        (att_outputs, att_finals), (outputs, finals) = stacks
        _, attended = _sigmoid_attention_fc(att_outputs, num_frames, 1, "RNN/fully_connected", l2_penalty, values_tm=outputs)
        final_state = torch.cat([attended.view(attended.shape[0], lstm_size)] + [c for c, _ in att_finals] + [c for c, _ in finals], dim=1)
        return _classify(final_state, model_input, vocab_size, **unused_params)


class LstmMultiAttentionModel(models.BaseModel):
    """W/all_frame_models/lstm_multi_attention_model.py:13-91: as LstmAttentionModel with --attention_size sigmoid attentions; each
    weighs the input frames (attention_input [B,A,D], the reference's einsum), the head runs on the B A rows and the prediction is the
    maximum over a video's A rows, as LstmAttentionMaxPoolingModel finishes.  Variables: RNN/multi_rnn_cell/cell_<l>/basic_lstm_cell/
    {weights,biases} and fully_connected/{weights,biases} (this FC sits outside the RNN scope; l2_penalty on the weights).  mask_emb is
    left out as in LstmAttentionModel.  accepts_quantized_input: the stack and the pooling read the reader's bytes."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        lstm_size = int(FLAGS.lstm_cells)
        attention_size = FLAGS.attention_size
        l2_penalty = unused_params.get("l2_penalty", 1e-8)
        model_input, _ = _bytes_or_floats(model_input, num_frames,
                                          lambda q: _lib_u8_ok(q.shape[2]) and seq_ops.u8_attention_supported(q, attention_size))
        out_tm, _ = _lstm_stack(model_input, num_frames, lstm_size, FLAGS.lstm_layers)
        attention, _ = _sigmoid_attention_fc(out_tm, num_frames, attention_size, "fully_connected", l2_penalty)
        attention_input = _attend_frames(attention, model_input, num_frames)                                  # [B,A,D]
        attention_output = _classify(attention_input.reshape(-1, model_input.shape[2]), model_input, vocab_size, **unused_params)["predictions"]
        final_output = ops.frame_pool(attention_output.view(-1, attention_size, vocab_size), "max")           # tf.reduce_max over the attentions
        return {"predictions": final_output}


def _parallel_stacks(model_input, num_frames, lstm_sizes, feature_sizes, number_of_layers, own_slots=False, scope_prefix="", slot_base=0):
    """One LSTM stack per input feature under scope <scope_prefix>RNN<i> (W/all_frame_models/lstm_parallel_finaloutput_model.py:34-64,
    lstm_cnn_deep_combine_chain_model.py:139-174): the input is split by feature_sizes and each part re-normalised; a part that arrives
    as bytes goes to _stack_input as bytes (see LstmParallelFinaloutputModel).  own_slots: stack i takes slot = slot_base + i -- for a
    caller that keeps the stacks' outputs alive together.  Returns [(top outputs time-major [F,B,H_i], finals)] per part."""
    assert sum(feature_sizes) == model_input.shape[2], "feature_sizes do not add up to the input width"
    res, off = [], 0
    for i, (fs, hs) in enumerate(zip(feature_sizes, lstm_sizes)):
        sub_input = model_input[:, :, off:off + fs].contiguous()
        if sub_input.dtype != torch.uint8:                        # (bytes: _stack_input reads them or dequantises + normalises the slice)
            sub_input = ops.l2_normalize(sub_input)
        off += fs
        res.append(_lstm_stack(sub_input, num_frames, hs, number_of_layers, scope="%sRNN%d" % (scope_prefix, i),
                               **(dict(slot=slot_base + i) if own_slots else {})))
    return res


class LstmParallelFinaloutputModel(models.BaseModel):
    """W/all_frame_models/lstm_parallel_finaloutput_model.py:13-73: one LSTM stack per input feature (rgb / audio: the
    input is split by --feature_sizes, each part re-normalised), head input = concat of every layer's final h.
    accepts_quantized_input: l2_normalize(slice of l2_normalize(x)) = l2_normalize(slice of x), so a stack whose slice the uint8
    projection covers reads the reader's bytes of that slice (its own row norms folded into the GEMM epilogue, see _lstm_stack); the
    other slices are dequantised and normalised as floats."""
    accepts_quantized_input = True

    def _head_extras(self, **unused_params):
        """(what stands behind the stacks' final h in the head input, the parameters left for the head)."""
        return [], unused_params

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        extras, unused_params = self._head_extras(**unused_params)
        lstm_sizes, feature_sizes = _sizes_per_feature()
        states = [h for _, finals in _parallel_stacks(model_input, num_frames, lstm_sizes, feature_sizes, FLAGS.lstm_layers) for _, h in finals]
        final_state = torch.cat(states + extras, dim=1)
        return _classify(final_state, model_input, vocab_size, **unused_params)


class LstmPositionalAttentionMaxPoolingModel(LstmAttentionMaxPoolingModel):
    """W/all_frame_models/lstm_positional_attention_max_pooling_model.py:10-87: as LstmAttentionMaxPoolingModel, the
    attention FC additionally sees a learned positional embedding [1,F,E] and the masked mean of the input."""

    def attention_parts(self, model_input, num_frames, l2_penalty):
        B, F, D = model_input.shape
        g = get_default_graph()
        emb = g.get_variable("positional_embedding", (1, F, FLAGS.positional_embedding_size), xavier_uniform, l2=l2_penalty)
        positional_embedding = ops.as_tensor(emb).expand(B, F, FLAGS.positional_embedding_size)
        if model_input.dtype == torch.uint8:
            # raw reader bytes: the masked mean frame from the bytes, the FC on [x | emb | mean | outputs] with x read as bytes and the
            # mean as ONE row per video
            rs = seq_ops.u8_frame_scales(model_input, num_frames)
            return [positional_embedding.contiguous(), _mean_frame(model_input, num_frames, rs)], rs
        return [positional_embedding, _mean_frame(model_input, num_frames)[:, None, :].expand(B, F, D)], None


def _cnn_filters(D, sub_scope, num_filters, filter_sizes, l2_penalty, name="cnn-filter-len%d", init=None):
    g = get_default_graph()
    return [g.get_variable(sub_scope + name % fs, (D * fs, nf), init or random_normal(0.1), l2=l2_penalty)
            for nf, fs in zip(num_filters, filter_sizes)]


def _einsum_cnn(model_input, fvars):
    """The reference's `cnn` on float frames [B,F,D] (cnn_deep_combine_chain_model.py:60-82, multiscale_cnn_lstm_model.py:12-38): per
    filter [fs D, N] one ops.linear on the input concatenated with its 1- .. (fs - 1)-frame shifts."""
    B, F, D = model_input.shape
    shift_inputs = [model_input]
    for i in range(1, max(W.data.shape[0] // D for W in fvars)):       # tf.pad(..., [[0,0],[i,0],[0,0]])[:, :F]
        shift_inputs.append(torch.cat([model_input.new_zeros(B, min(i, F), D), model_input[:, :max(F - i, 0)]], dim=1))
    outs = []
    for W in fvars:
        fs = W.data.shape[0] // D
        sub_input = torch.cat(shift_inputs[:fs], dim=2) if fs > 1 else shift_inputs[0]
        outs.append(ops.linear(sub_input.reshape(B * F, fs * D), W).view(B, F, -1))
    return torch.cat(outs, dim=2)


class CnnDeepCombineChainModel(models.BaseModel):
    """W/all_frame_models/cnn_deep_combine_chain_model.py:10-140: chain of MoE sub-predictions whose inputs are max-pooled
    "einsum CNNs" over the frames (filter lengths 1,2,3 = GEMMs on the input concatenated with its 1- and 2-frame shifts),
    the masked mean input and the l2-normalised relu projections of the previous predictions (the loop: video_level_models.prediction_chain
    with composed links; stage 0 reads cnn0 alone, a later stage [mean_input | cnn_k | mean-relu | relu-0 ..]).
    accepts_quantized_input: on the reader's bytes every CNN of the chain reads ONE half image of the frames (seq_ops.u8_cnn: a shift by
    i frames is a row offset in time-major order -- no concatenated [B,F,2D] / [B,F,3D] tensors, no fp32 copy of the frames), the mean
    frame comes from the bytes too."""
    accepts_quantized_input = True

    def cnn(self, model_input, l2_penalty=1e-8, num_filters=(1024, 1024, 1024), filter_sizes=(1, 2, 3), sub_scope="",
            **unused_params):
        return _einsum_cnn(model_input, _cnn_filters(model_input.shape[2], sub_scope, num_filters, filter_sizes, l2_penalty))

    def create_model(self, model_input, vocab_size, num_frames, num_mixtures=None, l2_penalty=1e-8, sub_scope="",
                     original_input=None, **unused_params):
        relu_cells = FLAGS.deep_chain_relu_cells
        model_input, frames, mean_input = self._frames_and_mean(model_input, num_frames)
        links = [relu_link(mean_input, relu_cells, sub_scope + "mean-relu", l2_penalty, composed_link("relu"))]
        frozen = 0 if mean_input.requires_grad else model_input.shape[2]      # the mean frame in front of a later stage's input is data

        def stage_input(k, links):                                  # cnn<k>'s variables are made here: after relu-<k - 1>
            cnn_output = self._pooled_cnn(model_input, frames, sub_scope + "cnn%d" % k, relu_cells, l2_penalty)
            return torch.cat([mean_input, cnn_output] + links, dim=1) if k else cnn_output

        return prediction_chain(self.sub_model, stage_input, composed_link("relu"), links, vocab_size, l2_penalty, sub_scope,
                                frozen_cols=lambda k: frozen if k else 0)

    def _frames_and_mean(self, model_input, num_frames):
        """(the frames as the chain's CNNs read them, their byte image -- ONE for every CNN of the chain, None for float frames --, the mean
        frame [B,D])."""
        model_input, u8 = _bytes_or_floats(model_input, num_frames, lambda q: seq_ops.u8_cnn_supported(q) and
                                           seq_ops.u8_attention_supported(q, 1))
        frames = seq_ops.U8FrameImages(model_input, num_frames) if u8 else None
        return model_input, frames, _mean_frame(model_input, num_frames)

    def _pooled_cnn(self, model_input, frames, scope, relu_cells, l2_penalty):
        """l2_normalize(reduce_max over the frames of the chain's CNN under `scope`) [B, 4 relu_cells]; frames: the byte image of the
        reader's bytes (seq_ops.U8FrameImages) or None for float frames."""
        filters = dict(num_filters=[relu_cells, relu_cells, relu_cells * 2], filter_sizes=[1, 2, 3])
        if frames is not None:
            fvars = _cnn_filters(model_input.shape[2], scope, l2_penalty=l2_penalty, **filters)
            if sum(filters["num_filters"]) % 4 == 0:                          # pooled in time-major order, sparse weight gradient
                return ops.l2_normalize(seq_ops.u8_cnn_maxpool(frames, fvars))
            cnn_output = seq_ops.u8_cnn(frames, fvars)
        else:
            cnn_output = self.cnn(model_input, sub_scope=scope, l2_penalty=l2_penalty, **filters)
        return ops.l2_normalize(ops.frame_pool(cnn_output, "max"))      # reduce_max over ALL max_frames rows, as the reference

    def sub_model(self, model_input, vocab_size, **params):
        return moe_stage(model_input, vocab_size, **params)


class DeepCnnDeepCombineChainModel(CnnDeepCombineChainModel):
    """W/all_frame_models/deep_cnn_deep_combine_chain_model.py:10-172: CnnDeepCombineChainModel whose stage k reads a three-level "deep CNN"
    deepcnn<k> instead of one CNN (c = --deep_cnn_base_size): level 0 the einsum CNN on the frames (filter lengths 1, 2, 3; c, c, 2c
    filters), levels 1 and 2 (lengths 2, 3; c filters each) on the max over frame pairs (tf.nn.pool MAX, window 2, stride 2, VALID) of
    the level before, F -> F // 2 -> F // 4 frames; the stage reads l2_normalize([max_t y0 | max_t y1 | max_t y2]) [B, 8c].  Padding
    frames are masked nowhere, as in the reference.  Unlike its sibling, tf.nn.dropout (--dropout) stands in front of EVERY stage,
    "-main" included (:119-120, 129-131); noise_level is accepted without effect.
    Variables in creation order: mean-relu, deepcnn0cnn<i>filter-len<fs>, gates-/experts-prediction-0, relu-0, deepcnn1.., gates-/experts--main.
    On the device everything is time-major (row t B + b): level 0 as seq_ops.u8_cnn_tm on ONE byte image of the frames shared by every
    deep CNN of the chain (seq_ops.cnn_tm on float frames), a level's two maxima from ONE pass over its output (seq_ops.max_pool2_tm,
    csrc/deep_cnn.hip), the last level as seq_ops.cnn_tm_maxpool, whose backward gathers.  CPU tensors take the batch-major composed form."""
    accepts_quantized_input = True

    LEVEL_FILTERS = ((1, 1, 2), (1, 1), (1, 1))                           # in units of --deep_cnn_base_size
    LEVEL_FILTER_SIZES = ((1, 2, 3), (2, 3), (2, 3))

    def create_model(self, model_input, vocab_size, num_frames, num_mixtures=None, dropout=False, keep_prob=None, noise_level=None,
                     l2_penalty=1e-8, sub_scope="", original_input=None, **unused_params):
        relu_cells, cnn_size = FLAGS.deep_chain_relu_cells, FLAGS.deep_cnn_base_size
        if model_input.shape[1] >> (len(self.LEVEL_FILTERS) - 1) == 0:
            raise ValueError("DeepCnnDeepCombineChainModel halves the frames twice: %d frames would leave a level without frames"
                             % model_input.shape[1])
        model_input, frames, mean_input = self._frames_and_mean(model_input, num_frames)
        links = [relu_link(mean_input, relu_cells, sub_scope + "mean-relu", l2_penalty, composed_link("relu"))]
        frozen = 0 if mean_input.requires_grad else model_input.shape[2]      # the mean frame in front of a later stage's input is data

        def stage_input(k, links):                                  # deepcnn<k>'s variables are made here: after relu-<k - 1>
            cnn_output = self._deep_cnn(model_input, frames, sub_scope + "deepcnn%d" % k, cnn_size, l2_penalty)
            return torch.cat([mean_input, cnn_output] + links, dim=1) if k else cnn_output

        def stage(x, vocab_size, **params):                         # the dropout reaches "-main" too: not prediction_chain's support_kwargs
            return self.sub_model(x, vocab_size, dropout=dropout, keep_prob=keep_prob, noise_level=noise_level, **params)

        return prediction_chain(stage, stage_input, composed_link("relu"), links, vocab_size, l2_penalty, sub_scope,
                                frozen_cols=lambda k: frozen if k else 0)

    def _deep_cnn(self, model_input, frames, scope, cnn_size, l2_penalty):
        """l2_normalize([reduce_max over the frames of every level's output]) [B, 8 cnn_size] of the deep CNN under `scope`; frames: the
        byte image of the reader's bytes (seq_ops.U8FrameImages) or None for float frames."""
        B, F, D = model_input.shape
        levels, d = [], D
        for i, (mult, sizes) in enumerate(zip(self.LEVEL_FILTERS, self.LEVEL_FILTER_SIZES)):
            levels.append(_cnn_filters(d, scope + "cnn%d" % i, [m * cnn_size for m in mult], sizes, l2_penalty, name="filter-len%d"))
            d = sum(mult) * cnn_size
        maxima = []
        if frames is not None or model_input.is_cuda:               # time-major rows t B + b throughout
            y = seq_ops.u8_cnn_tm(frames, levels[0]) if frames is not None else \
                seq_ops.cnn_tm(model_input.transpose(0, 1).reshape(F * B, D), B, levels[0])            # (layout glue)
            for fvars in levels[1:-1]:
                m, p = seq_ops.max_pool2_tm(y, F, B)
                maxima.append(m)
                F = F // 2
                y = seq_ops.cnn_tm(p.view(F * B, p.shape[2]), B, fvars)
            m, p = seq_ops.max_pool2_tm(y, F, B)
            maxima.append(m)
            F, x = F // 2, p.view((F // 2) * B, p.shape[2])
            if seq_ops.cnn_tm_maxpool_supported(x.shape[1], [levels[-1]]):                            # one frame per (video, column): gathers
                maxima.extend(seq_ops.cnn_tm_maxpool(x, B, [levels[-1]]))
            else:
                maxima.append(seq_ops.max_pool2_tm(seq_ops.cnn_tm(x, B, levels[-1]), F, B, want_pool=False)[0])
        else:                                                       # batch-major, composed, as the reference
            x = model_input
            for i, fvars in enumerate(levels):
                y = _einsum_cnn(x, fvars)
                maxima.append(y.amax(dim=1))
                if i + 1 < len(levels):
                    x = y[:, :(F // 2) * 2].reshape(B, F // 2, 2, y.shape[2]).amax(dim=2)
                    F = F // 2
        return ops.l2_normalize(torch.cat(maxima, dim=1))


class CnnLstmMemoryModel(models.BaseModel):
    """W/all_frame_models/cnn_lstm_memory_model.py:13-86: the einsum CNN (filter lengths 1, 2, 3 with 1024 filters each, fixed) on the
    frames, every frame's 3072 outputs l2-normalised, MultiRNNCell of --lstm_layers BasicLSTMCell(--lstm_cells) under dynamic_rnn; the
    head reads the concatenated c states.  Variables: cnn-filter-len{1,2,3}, RNN/multi_rnn_cell/cell_<l>/basic_lstm_cell/{weights,biases}.
    The CNN output rows num_frames and num_frames + 1 are non-zero (their windows reach live frames); dynamic_rnn never reads them and
    their gradient is zero.  On the device the CNN's output stays time-major (seq_ops.u8_cnn_tm on the reader's bytes, seq_ops.cnn_tm on
    floats) and IS, normalised, the native stack's float input [F,B,3072], which hands back the gradient to it."""
    accepts_quantized_input = True

    NUM_FILTERS = (1024, 1024, 1024)
    FILTER_SIZES = (1, 2, 3)

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        lstm_size = int(FLAGS.lstm_cells)
        number_of_layers = FLAGS.lstm_layers
        B, F, D = model_input.shape
        width = sum(self.NUM_FILTERS)
        x, u8 = _bytes_or_floats(model_input, num_frames, seq_ops.u8_cnn_supported)
        fvars = _cnn_filters(D, "", self.NUM_FILTERS, self.FILTER_SIZES, 1e-8)
        if u8 or x.is_cuda:
            y = seq_ops.u8_cnn_tm(seq_ops.U8FrameImages(x, num_frames), fvars) if u8 else \
                seq_ops.cnn_tm(x.transpose(0, 1).reshape(F * B, D), B, fvars)                          # (layout glue)
            x_tm = ops.l2_normalize(y).view(F, B, width)
        else:
            x_tm = ops.l2_normalize(_einsum_cnn(x, fvars).reshape(B * F, width)).view(B, F, width).transpose(0, 1).contiguous()
        with get_default_graph().variable_scope("RNN"):
            wb = _lstm_cells(width, lstm_size, number_of_layers)
        _, finals = _native_stack(x_tm, num_frames.to(torch.int32), wb)
        final_state = torch.cat([c for c, _ in finals], dim=1)
        return _classify(final_state, model_input, vocab_size, **unused_params)


def _pooled_cnn_chain(lstm_output_tm, cnns):
    """[reduce_max over ALL max_frames rows of cnn_c(lstm_output) [B, sum N]] for every CNN c of the chain, lstm_output_tm [F,B,D]
    time-major (padding rows zeros, as dynamic_rnn leaves them).  The ONE place the chain plugins' pooled CNNs go through: one op for the
    whole chain whose backward gathers (seq_ops.cnn_tm_maxpool).  Composed from the other plugins' ops it would be
    [seq_ops.cnn_tm(x, B, cnn).view(F, B, -1).amax(0) for cnn in cnns] -- what tests and tools/lstmcnn_step.py put here to compare."""
    F, B, D = lstm_output_tm.shape
    return seq_ops.cnn_tm_maxpool(lstm_output_tm.reshape(F * B, D), B, cnns)


class LstmCnnDeepCombineChainModel(models.BaseModel):
    """W/all_frame_models/lstm_cnn_deep_combine_chain_model.py:10-174: one LSTM stack per input feature (RNN<i>, as
    LstmParallelFinaloutputModel), their OUTPUTS concatenated [B,F,sum H_i] (zeros at frames >= num_frames); deep_chain_layers + 1 einsum CNNs
    (filter lengths 1, 2, 3; c, 2c, c filters for cnn0 and c, c, 2c for the others, c = --deep_chain_relu_cells) over that, each max-pooled
    over all max_frames rows and l2-normalised; a chain of MoE sub-predictions (prediction_chain): stage 0 reads cnn0 alone, stage l + 1 reads
    [cnn_{l+1} | mean-relu | relu-0 .. relu-l] (no mean_input columns, unlike CnnDeepCombineChainModel).  None of the CNNs depends on a
    prediction: they run as one op (_pooled_cnn_chain) on the stacks' time-major outputs, no transpose to batch-major.
    Variables: RNN<i>/multi_rnn_cell/cell_<l>/basic_lstm_cell/{weights,biases}, cnn<k>cnn-filter-len{1,2,3}, mean-relu, relu-<l>,
    gates-/experts-prediction-<l>, gates-/experts--main (the reference's constant mask_emb lookup table is num_frames arithmetic here).
    accepts_quantized_input: the stacks read their slices of the reader's bytes, the mean frame comes from the bytes too."""
    accepts_quantized_input = True

    def _first_relu_layers(self, l2_penalty, **unused_params):
        """What stands in relu_layers before mean-relu, and whether stage 0 already reads relu_layers."""
        return [], False

    def create_model(self, model_input, vocab_size, num_frames, num_mixtures=None, l2_penalty=1e-8, sub_scope="",
                     original_input=None, **unused_params):
        num_layers = FLAGS.deep_chain_layers
        relu_cells = FLAGS.deep_chain_relu_cells
        lstm_sizes, feature_sizes = _sizes_per_feature()
        links, early = self._first_relu_layers(l2_penalty, **unused_params)
        model_input, _ = _bytes_or_floats(model_input, num_frames, lambda q: seq_ops.u8_attention_supported(q, 1))
        mean_input = _mean_frame(model_input, num_frames)
        stacks = _parallel_stacks(model_input, num_frames, lstm_sizes, feature_sizes, FLAGS.lstm_layers, own_slots=True)
        lstm_output = torch.cat([out_tm for out_tm, _ in stacks], dim=2)                   # [F,B,sum H_i] time-major
        links.append(relu_link(mean_input, relu_cells, sub_scope + "mean-relu", l2_penalty, composed_link("relu")))
        D = lstm_output.shape[2]
        cnns = [_cnn_filters(D, sub_scope + "cnn%d" % k, [relu_cells, 2 * relu_cells, relu_cells] if k == 0 else
                             [relu_cells, relu_cells, 2 * relu_cells], [1, 2, 3], l2_penalty) for k in range(num_layers + 1)]
        pooled = [ops.l2_normalize(p) for p in _pooled_cnn_chain(lstm_output, cnns)]
        return prediction_chain(self.sub_model, lambda k, links: torch.cat([pooled[k]] + links, dim=1) if k or early else pooled[0],
                                composed_link("relu"), links, vocab_size, l2_penalty, sub_scope)

    def sub_model(self, model_input, vocab_size, **params):
        return moe_stage(model_input, vocab_size, **params)


class DistillchainLstmCnnDeepCombineChainModel(LstmCnnDeepCombineChainModel):
    """W/all_frame_models/distillchain_lstm_cnn_deep_combine_chain_model.py:10-105: LstmCnnDeepCombineChainModel whose relu_layers start
    with "distillrelu" (relu FC, --distillchain_relu_cells wide, over another model's predictions, l2-normalised) in front of mean-relu,
    and whose stage 0 already reads [cnn0 | relu_layers]."""

    def _first_relu_layers(self, l2_penalty, distillation_predictions=None, **unused_params):
        return [_distill_link(distillation_predictions, FLAGS.distillchain_relu_cells, l2_penalty, link=composed_link("relu"))], True


class DistillchainLstmParallelFinaloutputModel(LstmParallelFinaloutputModel):
    """W/all_frame_models/distillchain_lstm_parallel_finaloutput_model.py:13-88: LstmParallelFinaloutputModel whose head input is
    [final h of every layer of every stack | distill_norm] ("distillrelu", --distillchain_relu_cells wide, over another model's
    predictions).  Reads bytes on its parent's terms (_parallel_stacks)."""

    def _head_extras(self, distillation_predictions=None, l2_penalty=1e-8, **unused_params):
        return [_distill_link(distillation_predictions, FLAGS.distillchain_relu_cells, l2_penalty)], unused_params


class DistillchainCnnDeepCombineChainModel(CnnDeepCombineChainModel):
    """W/all_frame_models/distillchain_cnn_deep_combine_chain_model.py:10-148: relu_layers starts [distill_norm, mean_relu_norm] and every
    stage -- stage 0 included -- reads [normalized_cnn_output] + relu_layers: no mean_input columns in front, unlike this build's
    CnnDeepCombineChainModel.  distillrelu is --distillchain_relu_cells wide; mean-relu and relu-<l> go through ops.chain_link too.  The
    byte path (seq_ops.U8FrameImages, u8_cnn_maxpool) under the parent's conditions."""

    def create_model(self, model_input, vocab_size, num_frames, num_mixtures=None, l2_penalty=1e-8, sub_scope="",
                     original_input=None, distillation_predictions=None, **unused_params):
        relu_cells = FLAGS.deep_chain_relu_cells
        links = [_distill_link(distillation_predictions, FLAGS.distillchain_relu_cells, l2_penalty)]
        model_input, frames, mean_input = self._frames_and_mean(model_input, num_frames)
        links.append(relu_link(mean_input, relu_cells, sub_scope + "mean-relu", l2_penalty, fused_link("relu")))

        def stage_input(k, links):
            return torch.cat([self._pooled_cnn(model_input, frames, sub_scope + "cnn%d" % k, relu_cells, l2_penalty)] + links, dim=1)

        return prediction_chain(self.sub_model, stage_input, fused_link("relu"), links, vocab_size, l2_penalty, sub_scope)


class DistillchainLstmAttentionMaxPoolingModel(LstmAttentionMaxPoolingModel):
    """W/all_frame_models/distillchain_lstm_attention_max_pooling_model.py:10-116: LstmAttentionMaxPoolingModel whose sub_moe reads
    [attention_outputs | distill_norm tiled over the --lstm_attentions rows of a video] ("distillrelu", --distillchain_relu_cells wide).
    The rest is the parent's path, bytes included."""

    def create_model(self, model_input, vocab_size, num_frames, num_mixtures=None, l2_penalty=1e-8, sub_scope="",
                     distillation_predictions=None, original_input=None, **unused_params):
        self._distill_norm = _distill_link(distillation_predictions, FLAGS.distillchain_relu_cells, l2_penalty)
        try:
            return super().create_model(model_input, vocab_size, num_frames, num_mixtures=num_mixtures, l2_penalty=l2_penalty,
                                        sub_scope=sub_scope, original_input=original_input, **unused_params)
        finally:
            self._distill_norm = None

    def _moe_input(self, attention_outputs):
        B, A, _ = attention_outputs.shape
        tiled_distill_norm = self._distill_norm[:, None, :].expand(B, A, self._distill_norm.shape[1])
        return torch.cat([attention_outputs, tiled_distill_norm], dim=2)


def _memory_stacks(x_tm, d_in, num_frames, lstm_size, number_of_layers):
    """k -> [final c of every layer] of stack k of a multi-LSTM chain plugin: MultiRNNCell([BasicLSTMCell(H, forget_bias=1.0)] * L) under
    dynamic_rnn in variable_scope("lstm-<k>-RNN") (W/all_frame_models/lstm_memory_deep_chain_model.py:57-73; variables
    lstm-<k>-RNN/multi_rnn_cell/cell_<l>/basic_lstm_cell/{weights,biases}).  Every stack reads the SAME prepared input x_tm (_stack_input,
    made once by the caller) and owns slot k: the stacks' scratch and tapes are alive together until the backward pass."""
    g = get_default_graph()

    def memories(k):
        with g.variable_scope("lstm-%d-RNN" % k):
            wb = _lstm_cells(d_in, lstm_size, number_of_layers)
        _, finals = _native_stack(x_tm, num_frames, wb, slot=k)
        return [c for c, _ in finals]
    return memories


class LstmMemoryDeepChainModel(models.BaseModel):
    """W/all_frame_models/lstm_memory_deep_chain_model.py:13-104: deep_chain_layers + 1 LSTM stacks over the same frames (_memory_stacks),
    a prediction_chain of MoE sub-predictions: stage 0 reads the concatenated final memories of stack 0, stage l + 1 reads [memories of
    stack l + 1 | l2norm(relu-<l>(prediction-<l>))] -- only the latest relu, unlike the Combine form.  The concatenation is ops.memory_link,
    the relu -> l2norm ops.chain_link.  Variables: lstm-<k>-RNN/..., relu-<l>, gates-/experts-prediction-<l>, gates-/experts--main.
    accepts_quantized_input: every stack reads the reader's bytes (see _stack_input), prepared once."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, l2_penalty=1e-8, sub_scope="", original_input=None, **unused_params):
        memories = _memory_stacks(_stack_input(model_input, num_frames), model_input.shape[2], num_frames, int(FLAGS.lstm_cells),
                                  FLAGS.lstm_layers)

        def stage_input(k, links):                                  # stack k is built here: after relu-<k - 1>; only the latest link
            memory = ops.memory_link(memories(k), normalize=False)
            return torch.cat([memory, links[-1]], dim=1) if k else memory

        return prediction_chain(self.sub_moe, stage_input, fused_link("relu"), [], vocab_size, l2_penalty, sub_scope)

    def sub_moe(self, model_input, vocab_size, **params):
        return moe_stage(model_input, vocab_size, **params)


class DistillchainLstmMemoryDeepCombineChainModel(LstmMemoryDeepChainModel):
    """W/all_frame_models/distillchain_lstm_memory_deep_combine_chain_model.py:13-129: deep_chain_layers + 1 LSTM stacks over the same
    frames; relu_layers starts [distill_norm, mean_relu_norm] ("distill-relu" -- with a hyphen, unlike the other cascade plugins'
    distillrelu -- --distillchain_relu_cells wide over another model's predictions; "mean-relu" over the num_frames mean of the frames) and
    gains relu-<l> after stage l; every stage, stage 0 included, reads [l2norm(memories of stack k) | relu_layers...].  The normalised
    concatenation is ops.memory_link(normalize=True), every relu -> l2norm ops.chain_link.
    accepts_quantized_input: where the stack's byte projection and the byte pooling both cover the shape the stacks and the mean frame
    read the reader's bytes; else the frames are dequantised once for all of them."""

    def create_model(self, model_input, vocab_size, num_frames, l2_penalty=1e-8, sub_scope="", original_input=None,
                     distillation_predictions=None, **unused_params):
        links = [_distill_link(distillation_predictions, FLAGS.distillchain_relu_cells, l2_penalty, scope="distill-relu")]
        model_input, _ = _bytes_or_floats(model_input, num_frames, lambda q: _lib_u8_ok(q.shape[2]) and seq_ops.u8_attention_supported(q, 1))
        mean_input = _mean_frame(model_input, num_frames)
        links.append(relu_link(mean_input, FLAGS.deep_chain_relu_cells, sub_scope + "mean-relu", l2_penalty, fused_link("relu")))
        memories = _memory_stacks(_stack_input(model_input, num_frames), model_input.shape[2], num_frames, int(FLAGS.lstm_cells),
                                  FLAGS.lstm_layers)
        return prediction_chain(self.sub_moe, lambda k, links: torch.cat([ops.memory_link(memories(k), normalize=True)] + links, dim=1),
                                fused_link("relu"), links, vocab_size, l2_penalty, sub_scope)


class LstmParallelMemoryModel(models.BaseModel):
    """W/all_frame_models/lstm_parallel_memory_model.py:13-73: LstmParallelFinaloutputModel's stacks (one per input feature, RNN<i>), head
    input = every layer's final MEMORY c of every stack side by side (ops.memory_link over widths such as 1024, 1024, 128, 128).  Reads
    bytes on _parallel_stacks' terms."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        lstm_sizes, feature_sizes = _sizes_per_feature()
        stacks = _parallel_stacks(model_input, num_frames, lstm_sizes, feature_sizes, FLAGS.lstm_layers, own_slots=True)
        final_state = ops.memory_link([c for _, finals in stacks for c, _ in finals], normalize=False)
        return _classify(final_state, model_input, vocab_size, **unused_params)


def _time_major_stacks(parts_tm, num_frames, lstm_sizes, number_of_layers, scope_prefix, slot_base):
    """_parallel_stacks for parts that are prepared already: parts_tm[i] float32 [T, B, w_i] time-major and l2-normalised (a level of
    ops.frame_pyramid, or the hopped outputs of the level below).  Stack i runs under scope <scope_prefix>RNN<i> in slot slot_base + i;
    a part that requires a gradient gets one (the native stack's dx).  Returns [(top outputs [T,B,H_i], finals)]."""
    g = get_default_graph()
    res = []
    for i, (x_tm, hs) in enumerate(zip(parts_tm, lstm_sizes)):
        with g.variable_scope("%sRNN%d" % (scope_prefix, i)):
            wb = _lstm_cells(x_tm.shape[2], hs, number_of_layers)
        res.append(_native_stack(x_tm, num_frames, wb, slot=slot_base + i))
    return res


def _length_code(num_frames):
    """get_length_code of the temporal-pooling plugins: [B,5] one-hot float32 over num_frames <= 60, <= 120, <= 180, <= 240, > 240."""
    n = num_frames.view(-1, 1)
    edges = torch.tensor([60, 120, 180, 240], device=n.device, dtype=n.dtype)
    bucket = (n > edges).sum(dim=1)
    return torch.nn.functional.one_hot(bucket, 5).to(torch.float32)


class MultiresLstmMemoryDeepCombineChainModel(models.BaseModel):
    """W/all_frame_models/multires_lstm_memory_deep_combine_chain_model.py:13-165: DeepCombineChainModel's prediction_chain whose stage i reads
    the final memories of a fresh tower of per-feature LSTM stacks (lstm<i>RNN<j>, no hyphen) over the frames at resolution
    r_i = 2^(deep_chain_layers - i): the mean over every r frames, split by --feature_sizes, every part l2-normalised, num_frames // r
    steps.  next_input = [memories (stack-major, then layer) | length code with --deep_chain_use_length | l2norm(relu-<l>(prediction-<l>))
    of every earlier stage]; dropout on the support stages' inputs only.  Every level r >= 2 comes from ONE ops.frame_pyramid call, r = 1
    goes through _parallel_stacks; the memories of a stage are an ops.memory_link, every relu -> (noise) -> l2norm an ops.chain_link.
    accepts_quantized_input is False on purpose: elsewhere here uint8 frames at create_model stand for the DefaultTransformer's output
    (dequantised AND l2-normalised), and for this model the mean of normalised frames is not the mean of raw frames -- so the trainer folds
    nothing.  Under --feature_transformer=IdenticalTransformer (the training script's) the reader's bytes arrive as they are and mean
    what the reference's reader delivers: dequantised, padding zero, not normalised -- the pyramid kernel's path.  Under
    DefaultTransformer the model receives the normalised floats and averages those, as the reference would."""
    accepts_quantized_input = False

    def create_model(self, model_input, vocab_size, num_frames, num_mixtures=None, l2_penalty=1e-8, sub_scope="", original_input=None,
                     dropout=False, keep_prob=None, noise_level=None, **unused_params):
        num_layers = FLAGS.deep_chain_layers
        number_of_layers = FLAGS.lstm_layers
        lstm_sizes, feature_sizes = _sizes_per_feature()
        B, F, D = model_input.shape
        if F < (1 << num_layers):
            raise ValueError("MultiresLstmMemoryDeepCombineChainModel: %d frames are fewer than the coarsest resolution 2^%d: its LSTMs "
                             "would run over zero frames" % (F, num_layers))
        n = len(feature_sizes)
        seq_ops.reserve_resident((num_layers + 1) * n, number_of_layers)
        additional_features = [_length_code(num_frames)] if FLAGS.deep_chain_use_length else []
        parts, frames = ops.frame_pyramid(model_input, num_frames, num_layers, feature_sizes) if num_layers else ([], [])

        def memories(stage):
            level = num_layers - stage - 1                                  # resolution 2^(level + 1); -1: the frames themselves
            if level < 0:
                stacks = _parallel_stacks(model_input, num_frames, lstm_sizes, feature_sizes, number_of_layers, own_slots=True,
                                          scope_prefix="lstm%d" % stage, slot_base=stage * n)
            else:
                stacks = _time_major_stacks(parts[level], frames[level], lstm_sizes, number_of_layers, "lstm%d" % stage, stage * n)
            return ops.memory_link([c for _, finals in stacks for c, _ in finals], normalize=False)

        return prediction_chain(self.sub_model, lambda k, links: torch.cat([memories(k)] + links, dim=1),
                                fused_link(relu_kind(), noise_level), additional_features, vocab_size, l2_penalty, sub_scope,
                                support_kwargs=dict(dropout=dropout, keep_prob=keep_prob))

    def sub_model(self, model_input, vocab_size, **params):
        return moe_stage(model_input, vocab_size, **params)


class FramehopLstmMemoryModel(models.BaseModel):
    """W/all_frame_models/framehop_lstm_memory_model.py:13-126: a tower of per-feature LSTM stacks (lstm<k>RNN<i>), level 0 over the
    l2-normalised frames, level k >= 1 over l2norm(rows 1, 3, 5, .. of the top outputs of stack i of level k - 1): T_k = T_{k-1} // 2
    rows, input width and cells both H_i.  Every level k >= 1 is handed the ORIGINAL num_frames // 2 (:81), and dynamic_rnn runs no
    further than its input: min(num_frames // 2, T_k) steps, formed on the device.  Outputs past a video's length are zero rows and are
    hopped as they are.  Head input = every level's final memories, level-major, then stack, then layer (torch.cat: 20 tensors at the
    script's settings, more than ops.memory_link takes).  Gradients flow from every level through the hop into the level below.
    accepts_quantized_input: level 0 normalises per feature, so the bytes' two meanings agree, as in LstmParallelMemoryModel."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        if FLAGS.deep_chain_use_length:
            raise ValueError("FramehopLstmMemoryModel: --deep_chain_use_length reaches an undefined name (additional_features) in the "
                             "reference (framehop_lstm_memory_model.py:73); there is nothing to reproduce")
        num_layers = FLAGS.deep_chain_layers
        number_of_layers = FLAGS.lstm_layers
        lstm_sizes, feature_sizes = _sizes_per_feature()
        n = len(feature_sizes)
        seq_ops.reserve_resident((num_layers + 1) * n, number_of_layers)
        stacks = _parallel_stacks(model_input, num_frames, lstm_sizes, feature_sizes, number_of_layers, own_slots=True, scope_prefix="lstm0")
        states = [c for _, finals in stacks for c, _ in finals]
        half = torch.div(num_frames, 2, rounding_mode="floor")
        for k in range(1, num_layers + 1):
            T = stacks[0][0].shape[0] // 2
            if T < 1:
                raise ValueError("FramehopLstmMemoryModel: level %d of the tower has no frames left (%d at level 0)" % (k, model_input.shape[1]))
            hopped = [ops.l2_normalize(out[1:2 * T:2].contiguous()) for out, _ in stacks]
            stacks = _time_major_stacks(hopped, half.clamp(max=T), lstm_sizes, number_of_layers, "lstm%d" % k, k * n)
            states.extend(c for _, finals in stacks for c, _ in finals)
        final_states = torch.cat(states, dim=1)
        return _classify(final_states, model_input, vocab_size, num_frames=num_frames, **unused_params)


def _bn_vars(scope, n):
    g = get_default_graph()
    return (g.get_variable(scope + "/gamma", (n,), ones), g.get_variable(scope + "/beta", (n,), zeros),
            g.get_variable(scope + "/moving_mean", (n,), zeros, trainable=False),
            g.get_variable(scope + "/moving_variance", (n,), ones, trainable=False))


def _batch_norm(x, scope, is_training, eps=1e-3, decay=0.999):
    """slim.batch_norm(center=True, scale=True): batch moments, moving averages and the backward all in
    csrc/dbof.hip (ops.batch_norm).  Couples the examples of the local batch, like the reference."""
    return ops.batch_norm(x, *_bn_vars(scope, x.shape[-1]), is_training, eps, decay)


class MultiscaleCnnLstmModel(models.BaseModel):
    """W/all_frame_models/multiscale_cnn_lstm_model.py:10-137: --multiscale_cnn_lstm_layers scales; scale k runs the einsum CNN (filter
    lengths 1, 2, 3 with 256, 256, 512 filters) on its input [B, F_k, D_k], slim.batch_norm over ALL B F_k rows (padding frames included,
    as the reference), ReLU, one BasicLSTMCell under dynamic_rnn whose final memory c feeds a MoE, and hands the max over frame pairs of
    the ReLU output (F_{k+1} = F_k // 2, num_frames_{k+1} = max(num_frames_k // 2, 1)) to the next scale.  predictions = mean of the
    sub-predictions, support_predictions = their concatenation.  Variable names as TF 1.0 builds them, written from memory (as SURVEY.md
    Appendix A; pinned in tests/test_multiscale_host.py): cnn<k>cnn-filter-len{1,2,3}, cnn<k>cluster_bn/{gamma,beta,moving_mean,
    moving_variance}, RNN-rnn<k>/basic_lstm_cell/{weights,biases}, gatesmoe<k>/weights, expertsmoe<k>/{weights,biases}.

    Two paths, the same function and gradients.  fused (default on the device): every tensor of a scale stays time-major [F_k B, C]
    (row t B + b) -- the CNN as products on row windows (seq_ops.u8_cnn_tm on the reader's bytes at scale 1, seq_ops.cnn_tm on floats),
    batch norm + ReLU + pair maximum in one pass (seq_ops.bn_relu_pool2_tm, csrc/multiscale.hip) whose first output IS the native LSTM
    stack's input and whose second IS the next scale's.  generic (YT8M_MULTISCALE_FUSED=0, or shapes the fused kernels refuse): composed
    from ops.linear on shifted / concatenated inputs, ops.batch_norm and torch relu / amax, batch-major as the reference.
    accepts_quantized_input: scale 1 reads the reader's bytes through seq_ops.U8FrameImages where seq_ops.u8_cnn_supported holds."""
    accepts_quantized_input = True

    NUM_FILTERS = (256, 256, 512)
    FILTER_SIZES = (1, 2, 3)
    FILTER_INIT = None                       # _cnn_filters' default: tf.random_normal_initializer(stddev=0.1)
    SCALES_FLAG = "multiscale_cnn_lstm_layers"

    def _rnn(self, x_tm, num_frames, d_in, lstm_size, layer):
        g = get_default_graph()
        with g.variable_scope("RNN-rnn%d" % (layer + 1)):
            wb = _lstm_cells(d_in, lstm_size, 1, multi=False)
        _, finals = _native_stack(x_tm, num_frames, wb, slot=layer)                              # the L stacks are alive in one step
        return finals[0][0]                                                                      # state.c

    def moe(self, model_input, vocab_size, scopename="", **params):
        return moe_stage(model_input, vocab_size, sub_scope=scopename, hyphen=False, **params)

    def _head_input(self, lstm_memory):
        return lstm_memory

    def create_model(self, model_input, vocab_size, num_frames, l2_penalty=1e-8, is_training=True, **unused_params):
        sub_predictions, _ = self._scales(model_input, vocab_size, num_frames, FLAGS.multiscale_cnn_lstm_layers, l2_penalty, is_training)
        support_predictions = torch.cat(sub_predictions, dim=1)
        predictions = sub_predictions[0]
        for p in sub_predictions[1:]:
            predictions = predictions + p
        return {"predictions": predictions / float(len(sub_predictions)), "support_predictions": support_predictions}

    def _scales(self, model_input, vocab_size, num_frames, num_layers, l2_penalty, is_training):
        """The scale loop, shared with the LstmMultiscale plugins: ([sub-prediction [B,V] per scale], [lstm memory [B,H] per scale]).  Per
        scale the subclass's _rnn, _head_input (self._scale = the scale's index while it runs) and moe."""
        lstm_size = int(FLAGS.lstm_cells)
        is_training = bool(FLAGS.is_training and is_training)
        features_size = sum(self.NUM_FILTERS)
        B, F, D = model_input.shape
        model_input, u8 = _bytes_or_floats(model_input, num_frames, seq_ops.u8_cnn_supported)
        frames = seq_ops.U8FrameImages(model_input, num_frames) if u8 else None
        fused = seq_ops.MULTISCALE_FUSED and seq_ops.bn_relu_pool2_supported(model_input, features_size)
        nf = num_frames.to(torch.int32)
        # fused: cnn_input is time-major [F_k B, D_k]; generic: batch-major [B, F_k, D_k]
        cnn_input = None if frames is not None else (model_input.transpose(0, 1).reshape(F * B, D) if fused else model_input)
        sub_predictions, memories = [], []
        for layer in range(num_layers):
            scope = "cnn%d" % (layer + 1)
            self._scale = layer
            fvars = _cnn_filters(D, scope, self.NUM_FILTERS, self.FILTER_SIZES, l2_penalty, init=self.FILTER_INIT)
            gamma, beta, mm, mv = _bn_vars(scope + "cluster_bn", features_size)
            last = layer + 1 == num_layers
            if fused:
                y = seq_ops.u8_cnn_tm(frames, fvars) if (layer == 0 and frames is not None) else seq_ops.cnn_tm(cnn_input, B, fvars)
                relu_tm, pooled = seq_ops.bn_relu_pool2_tm(y, gamma, beta, mm, mv, is_training, F, B, want_pool=not last)
                next_input = None if last else pooled.view((F // 2) * B, features_size)
            else:
                if layer == 0 and frames is not None:
                    cnn_output = seq_ops.u8_cnn(frames, fvars)
                else:
                    cnn_output = _einsum_cnn(cnn_input, fvars)
                bn = ops.batch_norm(cnn_output.reshape(B * F, features_size), gamma, beta, mm, mv, is_training, 1e-3, 0.999)
                relu = torch.relu(bn).view(B, F, features_size)
                relu_tm = relu.transpose(0, 1).contiguous()
                next_input = None if last else relu[:, :(F // 2) * 2].reshape(B, F // 2, 2, features_size).amax(dim=2)
            lstm_memory = self._rnn(relu_tm, nf, features_size, lstm_size, layer)
            memories.append(lstm_memory)
            sub_predictions.append(self.moe(self._head_input(lstm_memory), vocab_size, l2_penalty=l2_penalty,
                                            scopename="moe%d" % (layer + 1)))
            cnn_input, F, D = next_input, F // 2, features_size
            nf = torch.clamp(nf // 2, min=1)                        # tf.maximum(num_frames / pool_size, 1), integer division
            if F == 0 and not last:
                raise ValueError("%s = %d needs more than %d frames" % (self.SCALES_FLAG, num_layers, model_input.shape[1]))
        return sub_predictions, memories


class DistillchainMultiscaleCnnLstmModel(MultiscaleCnnLstmModel):
    """W/all_frame_models/distillchain_multiscale_cnn_lstm_model.py:99-150: MultiscaleCnnLstmModel whose every MoE additionally reads the
    l2-normalised relu projection ("distillrelu", --distillchain_relu_cells wide) of another model's predictions, concatenated behind
    the LSTM memory."""

    def create_model(self, model_input, vocab_size, num_frames, distillation_predictions=None, l2_penalty=1e-8, **unused_params):
        self._distill_norm = _distill_link(distillation_predictions, FLAGS.distillchain_relu_cells, l2_penalty, link=composed_link("relu"))
        try:
            return super().create_model(model_input, vocab_size, num_frames, l2_penalty=l2_penalty, **unused_params)
        finally:
            self._distill_norm = None

    def _head_input(self, lstm_memory):
        return torch.cat([lstm_memory, self._distill_norm], dim=1)


class DbofModel(models.BaseModel):
    """W/all_frame_models/dbof_model.py:13-124: sample frames -> cluster FC -> (BN) -> relu6 -> pool over frames ->
    hidden FC -> (BN) -> relu6 -> head.  Weight variables are anonymous tf.Variable()s in the reference.

    accepts_quantized_input: raw uint8 frames are sampled FIRST (csrc/dbof.hip) and only the `iterations` sampled frames per
    video are dequantised + l2-normalised -- 30 of 300 rows; the fp32 [B,300,1152] tensor is never written."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, iterations=None, add_batch_norm=None,
                     sample_random_frames=None, cluster_size=None, hidden_size=None, is_training=True,
                     **unused_params):
        iterations = iterations or FLAGS.iterations
        add_batch_norm = add_batch_norm or FLAGS.dbof_add_batch_norm
        random_frames = sample_random_frames or FLAGS.sample_random_frames
        cluster_size = cluster_size or FLAGS.dbof_cluster_size
        hidden1_size = hidden_size or FLAGS.dbof_hidden_size
        g = get_default_graph()
        if random_frames:
            model_input = model_utils.SampleRandomFrames(model_input, num_frames, iterations)
        else:
            model_input = model_utils.SampleRandomSequence(model_input, num_frames, iterations)
        if model_input.dtype == torch.uint8:        # sampled frames are valid ones (all S, or none for a video without frames)
            nf_s = None if num_frames is None else (num_frames.to(torch.int32) > 0).to(torch.int32) * iterations
            model_input = ops.dequant_l2norm(model_input, nf_s)
        max_frames, feature_size = model_input.shape[1], model_input.shape[2]
        reshaped_input = model_input.reshape(-1, feature_size)
        if add_batch_norm:
            reshaped_input = _batch_norm(reshaped_input, "input_bn", is_training)
        cluster_weights = g.anonymous_variable((feature_size, cluster_size), random_normal(1 / math.sqrt(feature_size)))
        if add_batch_norm:
            activation = ops.linear(reshaped_input, cluster_weights)
            activation = _batch_norm(activation, "cluster_bn", is_training)
        else:
            cluster_biases = g.anonymous_variable((cluster_size,), random_normal(1 / math.sqrt(feature_size)))
            activation = ops.linear(reshaped_input, cluster_weights, cluster_biases)
        activation = ops.activation(activation, "relu6")
        activation = activation.view(-1, max_frames, cluster_size)
        activation = model_utils.FramePooling(activation, FLAGS.dbof_pooling_method)
        hidden1_weights = g.anonymous_variable((cluster_size, hidden1_size), random_normal(1 / math.sqrt(cluster_size)))
        if add_batch_norm:
            activation = ops.linear(activation, hidden1_weights)
            activation = _batch_norm(activation, "hidden1_bn", is_training)
        else:
            hidden1_biases = g.anonymous_variable((hidden1_size,), random_normal(0.01))
            activation = ops.linear(activation, hidden1_weights, hidden1_biases)
        activation = ops.activation(activation, "relu6")
        return _classify(activation, model_input, vocab_size, **unused_params)


class NetVLADModel(models.BaseModel):
    """soft-assignment + residual aggregation + intra-norm + L2 + hidden FC (+ context gating).

    accepts_quantized_input: the trainer may hand over the reader's RAW uint8 frames [B,F,D] instead of running the
    DefaultTransformer first; dequantise + l2-normalise are then folded into the pooling GEMMs (csrc/netvlad_fused.hip)
    and the fp32 [B,F,D] tensor is never written.  float inputs (or shapes the fused kernels do not cover) take the
    generic GEMM + softmax + batched-GEMM path; both give the same function."""
    gating = None
    accepts_quantized_input = True

    def descriptor(self, model_input, num_frames, cluster_size=None, hidden_size=None, gating=None):
        """[B,F,D] frames (uint8 raw or float transformed) -> hidden descriptor h [B, netvlad_hidden_size]."""
        K = cluster_size or FLAGS.netvlad_cluster_size
        Hfc = hidden_size or FLAGS.netvlad_hidden_size
        gating = (self.gating if self.gating is not None else FLAGS.netvlad_gating) if gating is None else gating
        g = get_default_graph()
        B, F, D = model_input.shape
        Wc = g.get_variable("netvlad/cluster_weights", (D, K), random_normal(1 / math.sqrt(D)))
        bc = g.get_variable("netvlad/cluster_biases", (K,), zeros)
        centres = g.get_variable("netvlad/centres", (K, D), random_normal(1 / math.sqrt(D)))
        # The descriptor-wide l2-normalisation needs no pass over [B,K,D]: the intra-normalised rows have the squared norms q
        # (1 unless clamped) the finishing kernel hands out, so v = vlad * s with s = rsqrt(max(sum_k q, eps)) per video, and
        # v . W = s * (vlad . W): the scale goes onto the [B, hidden] output (same function and gradients as l2_normalize first).
        want_q = seq_ops.vlad_q_supported(D)
        model_input, u8 = _bytes_or_floats(model_input, num_frames, lambda q: seq_ops.netvlad_fused_supported(q, K))
        if u8:
            nsplit = 1 if FLAGS.compute_dtype == "bfloat16" else 2        # f16 operands vs f16 hi+lo (fp32-class)
            vlad = seq_ops.netvlad_pool_u8(model_input, num_frames, Wc, bc, centres, nsplit, want_q=want_q)
        else:
            s = ops.linear(model_input, Wc, bc)                           # [B,F,K] assignment logits
            a = seq_ops.masked_softmax_rows(s, num_frames)                # softmax_k * mask
            agg = seq_ops.pool_tn(a, model_input)                         # [B,K,D] = a^T x per video
            vlad = seq_ops.vlad_finish(agg, a, centres, want_q=want_q)    # (agg - n*c), intra-normalised per cluster
        if want_q:
            vlad, qn = vlad
            scale = torch.rsqrt(torch.clamp(qn.sum(dim=1), min=1e-12)).unsqueeze(1)          # [B,1]; eps of ops.l2_normalize
            Wh = g.get_variable("netvlad/hidden/weights", (K * D, Hfc), video_level_models.xavier_uniform)
            bh = g.get_variable("netvlad/hidden/biases", (Hfc,), video_level_models.zeros)
            h = ops.linear(vlad.reshape(B, K * D), Wh, None) * scale + ops.as_tensor(bh)
        else:
            v = ops.l2_normalize(vlad.reshape(B, K * D))
            h = video_level_models.fully_connected(v, Hfc, "netvlad/hidden")
        if gating:
            gate = video_level_models.fully_connected(h, Hfc, "netvlad/gating", activation="sigmoid")
            h = h * gate
        return h

    def create_model(self, model_input, vocab_size, num_frames, cluster_size=None, hidden_size=None, gating=None,
                     **unused_params):
        h = self.descriptor(model_input, num_frames, cluster_size, hidden_size, gating)
        return _classify(h, model_input, vocab_size, **unused_params)


class GatedNetVLADModel(NetVLADModel):
    gating = True


class GatedNetVLADAttentionChainModel(GatedNetVLADModel):
    """BASELINE configs[4] composite ("Gated-NetVLAD + attention pooling + chained MoE"), fixed in SURVEY.md Appendix B
    from reference parts (NOT a reference class):
      (i)   h[b]       = gated NetVLAD descriptor (GatedNetVLADModel.descriptor);
      (ii)  att[b,a,:] = sum_f w[b,f,a] x[b,f,:],  w = renorm(mask * softmax_F([x || mean_x] W_a + b_a)) -- the attention
            pooling of W/all_frame_models/lstm_attention_max_pooling_model.py:34,51-63 with the LSTM outputs replaced by
            the frames themselves, A = --lstm_attentions;
      (iii) [h[b] || att[b,a]] -> DeepCombineChainModel (W/all_video_models/deep_combine_chain_model.py:12-85) on the
            [B*A] rows -> max over the A attentions (lstm_attention_max_pooling_model.py:64-66), for the predictions AND the
            support predictions so that they line up with MultiTaskCrossEntropyLoss.get_support (W/losses.py:225-255)."""

    def create_model(self, model_input, vocab_size, num_frames, l2_penalty=1e-8, **unused_params):
        A = FLAGS.lstm_attentions
        B, F, D = model_input.shape
        h = self.descriptor(model_input, num_frames)                                       # [B,Hfc] (uint8 stays fused)
        x, u8 = _bytes_or_floats(model_input, num_frames, lambda q: seq_ops.u8_attention_supported(q, A))
        if u8:
            # raw reader bytes all the way: the logit FC, the pooling and their gradients read uint8 (csrc/gemm_skinny.hip)
            rs = seq_ops.u8_frame_scales(x, num_frames)                                    # [B,F]; 0 on the padding frames
            mean_x = _mean_frame(x, num_frames, rs, clamp=True)
            g = video_level_models.get_default_graph()
            W = g.get_variable("attention-/weights", (2 * D, A), video_level_models.xavier_uniform, l2=l2_penalty)
            b = g.get_variable("attention-/biases", (A,), video_level_models.zeros)
            act = seq_ops.attention_logits_u8(x, rs, mean_x, W, b)
            w = seq_ops.attention_weights(act, num_frames)                                 # [B,F,A]
            att = seq_ops.pool_tn_u8(w, x, rs)                                             # [B,A,D]
        else:
            nf = num_frames.to(x.dtype).clamp(min=1).view(B, 1, 1) if num_frames is not None else float(F)
            mean_x = (x.sum(dim=1, keepdim=True) / nf).view(B, D)                          # tiled over the frames by the FC
            act = video_level_models.fully_connected_cat([x], A, "attention-", l2_penalty=l2_penalty, group_parts=[mean_x])
            w = seq_ops.attention_weights(act, num_frames)                                 # [B,F,A]
            att = seq_ops.pool_tn(w, x)                                                    # [B,A,D]
        chain_in = torch.cat([h.unsqueeze(1).expand(B, A, h.shape[1]), att], dim=2).reshape(B * A, -1)
        unused_params.pop("original_input", None)
        # max over the A attention rows of a video (lstm_attention_max_pooling_model.py:64-66), stage by stage: the support
        # predictions are pooled to [B, V] BEFORE they are concatenated (max over rows commutes with concatenation along columns)
        pool = lambda p_: ops.frame_pool(p_.view(B, A, vocab_size), "max")
        res = video_level_models.DeepCombineChainModel().create_model(chain_in, vocab_size, l2_penalty=l2_penalty,
                                                                      original_input=model_input, support_pool=pool, **unused_params)
        return {"predictions": pool(res["predictions"]), "support_predictions": res["support_predictions"]}


# ---- Z = youtube-8m-zhangteng: the scalar-gate LSTM models ------------------------------------------------------------------------
# Not built from Z/frame_level_models.py (one line each):
#   MoeDistillModel, MoeDistillEmbeddingModel (Z/video_level_models.py:157, :233): heads of the cascade family that are not in the final
#   submission's list (MoeDistillChainModel, -NormModel, -Norm2Model and MoeDistillSplitModel are built: video_level_models.py);
#   MoeDistillSplit2Model, MoeDistillSplit3Model, MoeDistillSplit4Model (Z/video_level_models.py:584 on): not in the list either;
#   CnnDCCDistillChainModel (entry 51, :6249): the plugin itself is not built, though the rule it is trained by, Z's calculate_loss_mix
#   on its predictions_class, now exists (train.TrainGraph._mix_loss);
#   MoeSoftmaxModel (entry 29.4) is built in video_level_models.py with its loss, losses.SplitSoftmaxLoss; of it, not built: `channels` other
#   than the reference's constant 1 (Z/video_level_models.py:920), and W's SoftmaxLoss / MultiTaskCrossEntropyAndSoftmaxLoss, a different
#   function (tf.nn.softmax of the predictions) under the name Z uses;
#   MoeMix4Model's --moe_group=True path (label groups of --class_size): no script of the list sets it;
#   Z's --distillation_type 1-3 losses: the cascade scripts say --distillation_type=0, the plain label loss;
#   of the random half-frame family (:4017, :6076-6247; built near the end of this file: LstmRandomModel, FrameRandomEvalModel,
#   FrameAttentionEvalModel), not built: VideoFrameEvalModel (:6076), which no script uses, and per-video rather than per-batch subsets;
#   LstmBiglu2Model: LstmBigluModel's pair of passes on LstmGlu2Model's input-memory cell (:1160), and not in the final submission's list;
#   LstmMultiscale3Model: LstmMultiscale2Model on LstmGlu2Model's input-memory cell with the HIDDEN state gathered at frame num_frames - 1,
#   not the memory (:3375, :3507): seq_ops.glu_lstm_layer hands back the gathered memory only, so it needs a second gather and its gradient;
#   LstmMultiscaleRebuildModel: a second training stage that fits ensemble_weight2d alone behind stop_gradient on restored scales; it has
#   no prediction_frames and needs the checkpoint hand-over between two models, which train.py does not have (:3592);
#   the other *Extend* models, each LstmExtendModel's attention (built at the end of this file, with InputExtendModel) with one change:
#   LstmExtendStateModel, LstmExtendCNNModel: the attention pools the outputs of a shifted-frames einsum CNN over the input (:5236, :5403);
#   LstmExtendInputModel: the attention pools the input frames themselves (:5336);
#   LstmExtendOrthoModel: calculate_ortho(W1) is added to the regularisation losses (:5503);
#   LstmGateExtendModel, LstmGluExtendModel: the outputs come from a scalar-gate / glu cell's while_loop, not dynamic_rnn (:5574, :5675);
#   LstmExtendParallelModel: an LSTM over the rgb part only, whose attention also pools the raw audio part (:5778).
GATE_LSTM_VARS = ("Wi", "Ui", "bi", "Wf", "Uf", "bf", "Wog", "Uog", "bog", "Wc", "Uc", "bc")      # create_recurrent_unit's order


def _scalar_gate_unit(names, d_in, hidden, l2_penalty, forget_bias=1.0, v_rows=None):
    """create_recurrent_unit of the scalar-gate cell (Z/frame_level_models.py:1583-1611, :1733-1761: GATE_LSTM_VARS) and of the
    input-memory cell (:695-749: GLU_LSTM_VARS) in the current scope: the Variables `names`, in that order, with the reference's names,
    shapes and initial values -- weights truncated_normal(stddev=0.1), the forget biases bf = bfx = forget_bias, the other biases 0.1
    -- every one of them, biases included, under l2_penalty * l2_loss.  W* act on the frame, V* on the l2-normalised input memory
    (v_rows None: d_in rows) or on whatever v_rows-wide tensor the calling cell feeds them, U* on h; the output gate "og" and the
    candidate "c" are `hidden` wide, every other gate is one scalar per video."""
    g = get_default_graph()

    def shape(n):
        width = hidden if n[1:] in ("og", "c") else 1
        rows = hidden if n[0] == "U" else (v_rows if n[0] == "V" and v_rows is not None else d_in)
        return (width,) if n[0] == "b" else (rows, width)

    def init(n):
        return truncated_normal(0.1) if n[0] != "b" else constant(forget_bias if n in ("bf", "bfx") else 0.1)

    return {n: g.get_variable(n, shape(n), init(n), l2=l2_penalty) for n in names}


def _gate_lstm_layer(x_tm, num_frames, hidden, scope, l2_penalty):
    """One layer under variable_scope(scope): the unit's Variables as views into the operands of seq_ops.gate_lstm_layer (concatenated
    per call: [Wog|Wc], [Wi|Wf], [Uog|Uc], [Ui|Uf]^T; the gradients come back through the same glue into each Variable's slot).
    Returns (out_tm [F,B,H], the memory gathered at frame num_frames - 1 [B,H])."""
    d_in = x_tm.D if isinstance(x_tm, seq_ops.U8FrameImages) else x_tm.shape[2]
    with get_default_graph().variable_scope(scope):
        v = {n: ops.as_tensor(var) for n, var in _scalar_gate_unit(GATE_LSTM_VARS, d_in, hidden, l2_penalty).items()}
    Wv, bv = torch.cat([v["Wog"], v["Wc"]], dim=1), torch.cat([v["bog"], v["bc"]])
    Ws, bs = torch.cat([v["Wi"], v["Wf"]], dim=1), torch.cat([v["bi"], v["bf"]])
    Uv, Us = torch.cat([v["Uog"], v["Uc"]], dim=1), torch.cat([v["Ui"], v["Uf"]], dim=1).t()
    return seq_ops.gate_lstm_layer(x_tm, Wv, bv, Ws, bs, Uv, Us, num_frames)


class _CellLayerModel(models.BaseModel):
    """One layer of a while_loop cell under "lstm_forward"; the head reads the gathered memory.  `layer` is the cell's layer function."""
    accepts_quantized_input = True
    layer = None

    def create_model(self, model_input, vocab_size, num_frames, l2_penalty=1e-8, **unused_params):
        x_tm = _hoisted_input(model_input, num_frames)
        _, state = self.layer(x_tm, num_frames, int(FLAGS.lstm_cells), "lstm_forward", l2_penalty)
        return _classify(state, model_input, vocab_size, **unused_params)


class _CellMultilayerModel(models.BaseModel):
    """--lstm_layers layers of a while_loop cell, layer i under "lstm_lsyer<i>lstm_forward"; the head reads the layers' gathered
    memories concatenated.  `layer` is the cell's layer function."""
    accepts_quantized_input = True
    layer = None

    def create_model(self, model_input, vocab_size, num_frames, l2_penalty=1e-8, **unused_params):
        hidden_outputs = _hoisted_input(model_input, num_frames)
        state_outputs = []
        for i in range(FLAGS.lstm_layers):
            # rnn_gate takes its own l2_penalty=1e-8 (Z/frame_level_models.py:1674, :826); create_model's is not forwarded to it
            hidden_outputs, state = self.layer(hidden_outputs, num_frames, int(FLAGS.lstm_cells), "lstm_lsyer%dlstm_forward" % i, 1e-8)
            state_outputs.append(state)
        return _classify(torch.cat(state_outputs, dim=1), model_input, vocab_size, **unused_params)


class LstmGateModel(_CellLayerModel):
    """Z/frame_level_models.py:1521-1640: one layer of the scalar-gate LSTM cell (input and forget gate one scalar per video, output
    gate and candidate vectors) run over all max_frames steps by a tf.while_loop -- no dynamic_rnn copy-through; the head
    (--video_level_classifier_model) reads the memory c gathered at frame num_frames - 1 (:1570-1574).  H = --lstm_cells.  Variables
    lstm_forward/{Wi,Ui,bi,Wf,Uf,bf,Wog,Uog,bog,Wc,Uc,bc}.  A row with num_frames < 1 (the reference gathers the previous video's last
    frame there, out of range for the first video) hands zeros to the head and receives no gradient.
    accepts_quantized_input: _hoisted_input -- the layer reads the reader's bytes where the byte products cover the shape."""
    layer = staticmethod(_gate_lstm_layer)


class LstmGateMultilayerModel(_CellMultilayerModel):
    """Z/frame_level_models.py:1642-1790: --lstm_layers layers of the scalar-gate cell (rnn_gate, :1674-1731); layer l + 1 reads all
    max_frames hidden outputs h of layer l, the head reads the layers' gathered memories concatenated (:1666).  Layer i's Variables
    live under "lstm_lsyer<i>lstm_forward/" -- the reference's spelling, which checkpoints carry.  Rows with num_frames < 1: as
    LstmGateModel.  accepts_quantized_input: _hoisted_input -- layer 0 reads the reader's bytes."""
    layer = staticmethod(_gate_lstm_layer)


DEFINE_integer("lstm_length", 10, "The length of each LSTM clip; only used in LstmLayerModel.")          # Z/frame_level_models.py: lstm_length


class LstmLayerModel(models.BaseModel):
    """Z/frame_level_models.py:3629-3683: a two-level LSTM.  Every video is cut into U2 = F // U1 clips of U1 = --lstm_length frames (the
    frames at or past U1 U2 are dropped, :3649-3651).  RNN-1: one BasicLSTMCell(H, forget_bias=1.0) in a MultiRNNCell under
    variable_scope("RNN-1") runs over all B U2 clips as one batch for U1 steps with sequence_length=None (:3653-3667): every row runs
    every step, padding frames are zero vectors.  RNN-2: the same cell construction under variable_scope("RNN-2"), with Variables of its
    own, runs over the U2 clip memories state_c of every video with sequence_length = num_frames // U1 (:3668-3675); the head
    (--video_level_classifier_model) reads its final memory [B, H] (:3677-3683).  H = --lstm_cells.  --lstm_layers is read and not used:
    both MultiRNNCells are built over range(1) (:3647, :3659).  Variable names, with this project's mapping of a scope-less dynamic_rnn
    (as for LstmModel): RNN-1/multi_rnn_cell/cell_0/basic_lstm_cell/{weights [D + H, 4H], biases [4H]} and
    RNN-2/multi_rnn_cell/cell_0/basic_lstm_cell/{weights [2H, 4H], biases [4H]}.  A video with num_frames < U1 hands zeros to the head,
    as dynamic_rnn does at length 0.
    accepts_quantized_input: RNN-1 (seq_ops.lstm_clip_layer) reads the reader's bytes where the byte projection covers the width."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, **unused_params):
        lstm_size = int(FLAGS.lstm_cells)
        unit_layer_1 = FLAGS.lstm_length
        g = get_default_graph()
        frames, _ = _bytes_or_floats(model_input, num_frames, lambda q: q.is_cuda and _lib_u8_ok(q.shape[2]))
        with g.variable_scope("RNN-1"):
            (W1, b1), = _lstm_cells(model_input.shape[2], lstm_size, 1)
        with g.variable_scope("RNN-2"):
            wb2 = _lstm_cells(lstm_size, lstm_size, 1)
        state_c = seq_ops.lstm_clip_layer(frames, num_frames, unit_layer_1, ops.as_tensor(W1), ops.as_tensor(b1))    # [U2, B, H]
        _, finals = _native_stack(state_c, num_frames // unit_layer_1, wb2, slot=1)
        return _classify(finals[0][0], model_input, vocab_size, **unused_params)


BIGATE_LSTM_BW_VARS = ("Wi", "Ui", "Vi", "bi", "Wf", "Vf", "Uf", "bf", "Wog", "Vog", "Uog", "bog", "Wc", "Vc", "Uc", "bc")   # :1036-1070


class LstmBigluModel(models.BaseModel):
    """Z/frame_level_models.py:887-1158: two passes of the scalar-gate LSTM cell, each a tf.while_loop over all max_frames steps.  The
    first (create_forward_recurrent_unit, Variables lstm_forward/{Wi,Ui,bi,Wf,Uf,bf,Wog,Uog,bog,Wc,Uc,bc}) reads
    tf.reverse_sequence(model_input, num_frames); tf.reverse_sequence of its hidden outputs, y, enters every gate of the second
    (create_backward_recurrent_unit, lstm_backward/{Wi,Ui,Vi,bi,Wf,Vf,Uf,bf,Wog,Vog,Uog,bog,Wc,Vc,Uc,bc}) through V*, which runs over
    the frames in order.  The head is the model's own sub_moe (--moe_num_mixtures, gatesbackward / expertsbackward; never
    --video_level_classifier_model) on [c1 | c2], both memories gathered at step num_frames - 1 (:939-943, :967-968).  H = --lstm_cells.
    Against LstmGateModel: bf starts at 0.1 in both units (:988, :1051), V* are [H,1] / [H,H] (they act on y), and sub_moe takes its
    own l2_penalty of 1e-8.  A row with num_frames < 1 hands zeros to the head and receives no gradient (as LstmGateModel).
    accepts_quantized_input: _hoisted_input -- both passes read the reader's bytes through one operand image where the byte products
    cover the shape (seq_ops.bigate_lstm_layer)."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, l2_penalty=1e-8, **unused_params):
        hidden = int(FLAGS.lstm_cells)
        x_tm = _hoisted_input(model_input, num_frames)
        d_in = x_tm.D if isinstance(x_tm, seq_ops.U8FrameImages) else x_tm.shape[2]
        g = get_default_graph()
        with g.variable_scope("lstm_forward"):
            fw = {n: ops.as_tensor(var) for n, var in _scalar_gate_unit(GATE_LSTM_VARS, d_in, hidden, l2_penalty, forget_bias=0.1).items()}
        with g.variable_scope("lstm_backward"):
            bw = {n: ops.as_tensor(var) for n, var in
                  _scalar_gate_unit(BIGATE_LSTM_BW_VARS, d_in, hidden, l2_penalty, forget_bias=0.1, v_rows=hidden).items()}
        # the units' Variables as views into the op's operands, as _gate_lstm_layer: the gradients come back through the same glue
        Wv, bv = torch.cat([fw["Wog"], fw["Wc"], bw["Wog"], bw["Wc"]], dim=1), torch.cat([fw["bog"], fw["bc"], bw["bog"], bw["bc"]])
        Ws, bs = torch.cat([fw["Wi"], fw["Wf"], bw["Wi"], bw["Wf"]], dim=1), torch.cat([fw["bi"], fw["bf"], bw["bi"], bw["bf"]])
        Uv1, Us1 = torch.cat([fw["Uog"], fw["Uc"]], dim=1), torch.cat([fw["Ui"], fw["Uf"]], dim=1).t()
        Uv2, Us2 = torch.cat([bw["Uog"], bw["Uc"]], dim=1), torch.cat([bw["Ui"], bw["Uf"]], dim=1).t()
        Vv, Vs = torch.cat([bw["Vog"], bw["Vc"]], dim=1), torch.cat([bw["Vi"], bw["Vf"]], dim=1)
        _, _, c1, c2 = seq_ops.bigate_lstm_layer(x_tm, Wv, bv, Ws, bs, Uv1, Us1, Vv, Vs, Uv2, Us2, num_frames)
        # sub_moe(moe_input, vocab_size, scopename="backward") (:970, :1104-1158): its own l2_penalty = 1e-8, "gates" + scopename
        return {"predictions": moe_stage(torch.cat([c1, c2], dim=1), vocab_size, l2_penalty=1e-8, sub_scope="backward", hyphen=False)}


# ---- Z: the input-memory LSTM models (LstmGlu2Model, LstmGlu2MultilayerModel) -----------------------------------------------------
GLU_LSTM_VARS = ("Wi", "Ui", "Vi", "bi", "Wf", "Vf", "Uf", "bf", "Wog", "Vog", "Uog", "bog", "Wc", "Vc", "Uc", "bc",
                 "Wix", "Vix", "Uix", "bix", "Wfx", "Vfx", "Ufx", "bfx")                       # create_recurrent_unit's order


def _glu_lstm_layer(x_tm, num_frames, hidden, scope, l2_penalty):
    """One layer under variable_scope(scope): the unit's Variables as views into the operands of seq_ops.glu_lstm_layer (concatenated
    per call, as _gate_lstm_layer: [Wog|Wc], [Vog|Vc], [Uog|Uc] and the four scalar gates' columns in the order i, f, ix, fx; the
    gradients come back through the same glue into each Variable's slot).  Returns (out_tm [F,B,H], the memory gathered at frame
    num_frames - 1 [B,H])."""
    d_in = x_tm.D if isinstance(x_tm, seq_ops.U8FrameImages) else x_tm.shape[2]
    with get_default_graph().variable_scope(scope):
        v = {n: ops.as_tensor(var) for n, var in _scalar_gate_unit(GLU_LSTM_VARS, d_in, hidden, l2_penalty).items()}
    sc = ("i", "f", "ix", "fx")
    Wv, Vv, Uv = (torch.cat([v[k + "og"], v[k + "c"]], dim=1) for k in "WVU")
    Ws, Vs, Us = (torch.cat([v[k + n] for n in sc], dim=1) for k in "WVU")
    bv, bs = torch.cat([v["bog"], v["bc"]]), torch.cat([v["b" + n] for n in sc])
    return seq_ops.glu_lstm_layer(x_tm, Wv, bv, Ws, bs, Vv, Vs, Uv, Us.t(), num_frames)


class LstmGlu2Model(_CellLayerModel):
    """Z/frame_level_models.py:631-792: one layer of the input-memory LSTM cell -- the scalar-gate cell (LstmGateModel) with a second
    recurrent state over the INPUT, x_prev' = fx x_prev + ix x under two more scalar gates, whose l2-normalised value enters all six
    gates through V* -- run over all max_frames steps by a tf.while_loop; the head (--video_level_classifier_model) reads the memory
    c gathered at frame num_frames - 1 (:682-686).  H = --lstm_cells.  Variables lstm_forward/{Wi,Ui,Vi,bi,Wf,Vf,Uf,bf,Wog,Vog,Uog,bog,
    Wc,Vc,Uc,bc,Wix,Vix,Uix,bix,Wfx,Vfx,Ufx,bfx}.  A row with num_frames < 1 hands zeros to the head and receives no gradient (as
    LstmGateModel).  accepts_quantized_input: _hoisted_input -- the layer reads the reader's bytes where the byte products cover the
    shape."""
    layer = staticmethod(_glu_lstm_layer)


class LstmGlu2MultilayerModel(_CellMultilayerModel):
    """Z/frame_level_models.py:794-885: --lstm_layers layers of the input-memory cell (rnn_gate, :826-885); layer l + 1 reads all
    max_frames hidden outputs h of layer l, the head reads the layers' gathered memories concatenated (:818).  Layer i's Variables
    live under "lstm_lsyer<i>lstm_forward/" -- the reference's spelling, which checkpoints carry.  Rows with num_frames < 1: as
    LstmGlu2Model.  accepts_quantized_input: _hoisted_input -- layer 0 reads the reader's bytes."""
    layer = staticmethod(_glu_lstm_layer)


# ---- Z: the Extend attention models (LstmExtendModel, InputExtendModel) ------------------------------------------------------------
def _extend_variables(lstm_size, d_in, num_extend, l2_penalty):
    """W1 [H,E], b1 [E], W2 [D,E], b2 [E] at the top level, in the reference's order (Z/frame_level_models.py:5210-5217): weights
    truncated_normal(stddev=0.1), biases 0.1, every one of the four, biases included, under l2_penalty * l2_loss."""
    g = get_default_graph()
    return (g.get_variable("W1", (lstm_size, num_extend), truncated_normal(0.1), l2=l2_penalty),
            g.get_variable("b1", (num_extend,), constant(0.1), l2=l2_penalty),
            g.get_variable("W2", (d_in, num_extend), truncated_normal(0.1), l2=l2_penalty),
            g.get_variable("b2", (num_extend,), constant(0.1), l2=l2_penalty))


def _extend_input_logits(model_input, num_frames, W2, b2):
    """xw_plus_b(rnn_input, W2, b2) as [B,F,E], the `extra` operand of seq_ops.softmax_attention_tm: on the reader's bytes one skinny
    product over them (b2 on the padding frames, whose dequantised rows are zero), on float frames ops.linear.  The frames are data:
    the gradient goes to W2 and b2 only."""
    B, F, D = model_input.shape
    if model_input.dtype == torch.uint8:
        return seq_ops.attention_logits_u8(model_input, seq_ops.u8_frame_scales(model_input, num_frames), None, W2, b2, parts=[])
    if model_input.is_cuda:
        return ops.linear(model_input.reshape(B * F, D), W2, b2).view(B, F, -1)
    return (model_input.reshape(B * F, D) @ ops.as_tensor(W2) + ops.as_tensor(b2)).view(B, F, -1)


class LstmExtendModel(models.BaseModel):
    """Z/frame_level_models.py:5169-5234: an LSTM stack under RNN; --moe_num_extend attention heads, each a softmax OVER THE FRAMES of
    outputs . W1 + b1 + input . W2 + b2, times the mask of the video's frames and divided by its sum, pool the stack's top outputs
    into [B, E, H]; the head (--video_level_classifier_model, MoeExtendModel in the scripts) runs on the B E rows.  The result also
    carries "attention_weight" [B, E F] in the reference's head-major order, detached.  Variables: RNN/multi_rnn_cell/cell_<l>/
    basic_lstm_cell/{weights,biases}, then W1, b1, W2, b2 at the top level (see _extend_variables).  create_model's own l2_penalty
    reaches those four and, as in the reference, is not forwarded to the head.
    The mask: the reference takes frames_bool = (sum |x| > 0) per frame; float frames get exactly that.  On the reader's bytes a
    dequantised real frame is never all zero (127 * 4 / 255 - 2 + 4 / 512 != 0), so frames_bool is t < num_frames and the window
    hi = num_frames - 1 states it.  A video without a frame is NaN in the reference; here its attention and pooled rows are zero and it
    neither receives nor sends a gradient (seq_ops.softmax_attention_tm).
    accepts_quantized_input: the stack (see _lstm_stack) and the input logits read the reader's bytes; logits, softmax, mask and the
    pooling are one pass over the stack's time-major outputs in the shared mode of seq_ops.softmax_attention_tm."""
    accepts_quantized_input = True

    def _pooled_rows(self, model_input, num_frames, l2_penalty):
        """(the B E attention-pooled rows [B E, H], the input as the stack read it, the attention [B, F, E])"""
        lstm_size = int(FLAGS.lstm_cells)
        num_extend = FLAGS.moe_num_extend
        model_input, u8 = _bytes_or_floats(model_input, num_frames,
                                           lambda q: _lib_u8_ok(q.shape[2]) and seq_ops.u8_attention_supported(q, num_extend))
        B, F, D = model_input.shape
        out_tm, _ = _lstm_stack(model_input, num_frames, lstm_size, FLAGS.lstm_layers)
        W1, b1, W2, b2 = _extend_variables(lstm_size, D, num_extend, l2_penalty)
        extra = _extend_input_logits(model_input, num_frames, W2, b2)
        if u8:
            mask = dict(hi=(num_frames.to(torch.int32) - 1).view(B, 1).expand(B, num_extend).contiguous())
        else:
            mask = dict(valid=(model_input.abs().sum(dim=2) > 0).to(torch.uint8))
        attention, pooled = seq_ops.softmax_attention_tm(out_tm, W1, b1, out_tm, extra=extra, **mask)
        return pooled.reshape(B * num_extend, lstm_size), model_input, attention

    def create_model(self, model_input, vocab_size, num_frames, l2_penalty=1e-8, **unused_params):
        pooled, model_input, attention = self._pooled_rows(model_input, num_frames, l2_penalty)
        B, F, E = attention.shape
        result = _classify(pooled, model_input, vocab_size, **unused_params)
        result["attention_weight"] = attention.detach().transpose(1, 2).reshape(B, E * F)
        return result


class LstmExtendCombineModel(LstmExtendModel):
    """Z/frame_level_models.py:5852-5924: LstmExtendModel's stack and attention pooling, on the reader's bytes on LstmExtendModel's
    terms, with video_level_models.MoeMix4Model -- always that head, as in the reference -- on the B E pooled rows; its "predictions"
    and every stage's [B E, V] piece of its "predictions_class" are reduced by the maximum over a video's E rows (each piece is pooled
    before the concatenation: the maximum over rows commutes with it), so the result is trained by Z's mix loss
    (train.TrainGraph._mix_loss).  The scripts run it with --frame_features, which leaves the head's class inputs unnormalised.  The
    reference does not return "attention_weight" here; neither does this."""

    def create_model(self, model_input, vocab_size, num_frames, l2_penalty=1e-8, **unused_params):
        num_extend = FLAGS.moe_num_extend
        pooled, model_input = self._pooled_rows(model_input, num_frames, l2_penalty)[:2]
        unused_params.pop("original_input", None)
        pool = lambda p_: ops.frame_pool(p_.view(-1, num_extend, vocab_size), "max")        # tf.reduce_max over a video's rows
        return video_level_models.MoeMix4Model().create_model(pooled, vocab_size, original_input=model_input, support_pool=pool,
                                                              **unused_params)


def input_extend_windows(num_frames, num_extend):
    """(lo, hi) int32 [B,E], both ends included: lo = (num_frames // E) i, hi = lo + 2 (num_frames // E) (Z/frame_level_models.py:
    6022-6030).  num_frames = 0 gives [0, 0] for every head."""
    step = (num_frames.to(torch.int32) // num_extend).view(-1, 1)
    lo = step * torch.arange(num_extend, dtype=torch.int32, device=num_frames.device).view(1, -1)
    return lo.contiguous(), (lo + 2 * step).contiguous()


class InputExtendModel(models.BaseModel):
    """Z/frame_level_models.py:5995-6073: two LSTM stacks over the same input, RNN_Attention and RNN; --moe_num_extend attention heads,
    each a softmax over the frames of outputs(RNN_Attention) . W1 + b1 + input . W2 + b2 restricted to the head's window of frames
    [(num_frames // E) i, (num_frames // E) (i + 2)], pool the RNN stack's top outputs into [B, E, H]; the head runs on the B E rows.
    Variables: {RNN_Attention,RNN}/multi_rnn_cell/cell_<l>/basic_lstm_cell/{weights,biases}, then W1, b1, W2, b2 (_extend_variables).
    The mask is the window alone: the reference computes frames_bool_all, the mask of the empty frames, and never uses it, so the last
    windows run past num_frames ((E + 1) (num_frames // E) can exceed it).  There the stacks' rows are zero, the logit is b1 + b2, and
    those frames take their share of the softmax while adding zeros to the pooled rows.  That is reproduced.  num_frames = 0 gives the
    window [0, 0]: frame 0 takes all the weight and the pooled rows are zero.
    accepts_quantized_input: both stacks (slots of their own, as LstmAttentionLstmModel) and the input logits read the reader's bytes."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, l2_penalty=1e-8, **unused_params):
        lstm_size = int(FLAGS.lstm_cells)
        number_of_layers = FLAGS.lstm_layers
        num_extend = FLAGS.moe_num_extend
        g = get_default_graph()
        model_input, _ = _bytes_or_floats(model_input, num_frames,
                                          lambda q: _lib_u8_ok(q.shape[2]) and seq_ops.u8_attention_supported(q, num_extend))
        B, F, D = model_input.shape
        x_tm = _stack_input(model_input, num_frames)                 # prepared once, read by both stacks
        seq_ops.reserve_resident(2, number_of_layers)
        stacks = []
        for slot, scope in enumerate(("RNN_Attention", "RNN")):      # both stacks' outputs are alive together: slots of their own
            with g.variable_scope(scope):
                wb = _lstm_cells(D, lstm_size, number_of_layers)
            stacks.append(_native_stack(x_tm, num_frames, wb, slot=slot))
        (outputs, _), (outputs_features, _) = stacks
        W1, b1, W2, b2 = _extend_variables(lstm_size, D, num_extend, l2_penalty)
        extra = _extend_input_logits(model_input, num_frames, W2, b2)
        lo, hi = input_extend_windows(num_frames, num_extend)
        _, pooled = seq_ops.softmax_attention_tm(outputs, W1, b1, outputs_features, extra=extra, lo=lo, hi=hi)
        return _classify(pooled.reshape(B * num_extend, lstm_size), model_input, vocab_size, **unused_params)


# ---- Z: random half-frame inference (LstmRandomModel, FrameRandomEvalModel, FrameAttentionEvalModel) -------------------------------
# VideoFrameEvalModel (Z/frame_level_models.py:6076-6131), the fourth class of the family, is not built: no script uses it.
DEFINE_bool("lstm_random_frames", False, "LstmRandomModel: run every TRAINING step on one random, order-preserving half of the frames "
            "(what the reference's test FLAGS.train==\"train\" was written to do and, comparing a bool flag with a string, never does).")


def _random_halves(model_input, num_frames, replicas, seed):
    """(frames [B E, F // 2, D], num_frames [B E]): E replicas of every video, replica e on the e-th random half of the frame indices
    (ops.frame_subset: one order-preserving F // 2 subset per replica, shared by the batch; row b E + e = replica e of video b).  On
    the reader's bytes and on float frames alike; a replica's chosen padding frames are zero rows behind its real ones."""
    y, nf, _ = ops.frame_subset(model_input, num_frames, replicas, seed=seed)
    return y, nf


def _mean_over_replicas(predictions, replicas):
    """tf.reduce_mean(reshape(predictions, [-1, E, V]), axis=1)"""
    rows, V = predictions.shape
    return ops.frame_pool(predictions.reshape(rows // replicas, replicas, V), "average")


class LstmRandomModel(LstmMemoryModel):
    """Z/frame_level_models.py:4017-4079: LstmMemoryModel's function and variables (RNN/multi_rnn_cell/cell_<l>/basic_lstm_cell/
    {weights,biases}, then the head's).  The reference selects a random half of the frames behind `FLAGS.train=="train"`; --train is a
    bool flag (:54), so the test never holds and the model as committed is LstmMemoryModel in training and in evaluation alike.
    --lstm_random_frames=False (the default) is that.  True runs every training step (is_training) on one random, order-preserving half
    of the frames (E = 1, K = F // 2: ops.frame_subset), which is what the final submission's list says the model was trained with;
    evaluation and inference never select, as under the scripts' --train=False.  frame_subset_seed: the key of the draw (default: the
    graph's next random-op key)."""

    def create_model(self, model_input, vocab_size, num_frames, is_training=True, frame_subset_seed=None, **unused_params):
        if FLAGS.lstm_random_frames and is_training:
            model_input, num_frames = _random_halves(model_input, num_frames, 1, frame_subset_seed)
        if not is_training:
            unused_params["is_training"] = False
        return super().create_model(model_input, vocab_size, num_frames, **unused_params)


class FrameRandomEvalModel(models.BaseModel):
    """Z/frame_level_models.py:6182-6247, the test-time augmentation of LstmRandomModel's checkpoints: E = --moe_num_extend replicas of
    every video, each on a random, order-preserving half of its frames (unconditionally: this is an inference plugin), go through
    LstmMemoryModel's function as ONE batch of B E rows of F // 2 frames; the head reads the concatenated final memories and the
    predictions are averaged over a video's E rows.  Variables: exactly LstmMemoryModel's names and shapes, so a checkpoint trained as
    LstmMemoryModel or LstmRandomModel loads.  A replica that keeps none of a video's frames runs at length 0 and hands the zero state
    to the head, as dynamic_rnn does.  frame_subset_seed: the key of the draw (default: the graph's next random-op key).  The labels
    are not forwarded: the head sees B E rows.
    accepts_quantized_input: the replicas are gathered from the reader's bytes and the stack reads them (see _lstm_stack)."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, frame_subset_seed=None, **unused_params):
        num_extend = FLAGS.moe_num_extend
        unused_params.pop("labels", None)
        model_input, num_frames = _random_halves(model_input, num_frames, num_extend, frame_subset_seed)
        result = LstmMemoryModel().create_model(model_input, vocab_size, num_frames, **unused_params)
        return {"predictions": _mean_over_replicas(result["predictions"], num_extend)}


class FrameAttentionEvalModel(models.BaseModel):
    """Z/frame_level_models.py:6133-6180, the same test-time augmentation in front of LstmExtendModel().create_model: its predictions on
    the B E replicas are clipped to [0, 1] and averaged over a video's E rows.  As in the reference the one flag --moe_num_extend is both
    the number of replicas and LstmExtendModel's number of attention heads.  Variables: LstmExtendModel's.  frame_subset_seed and the
    labels: as FrameRandomEvalModel.
    accepts_quantized_input: the replicas are gathered from the reader's bytes, which LstmExtendModel reads on its own terms."""
    accepts_quantized_input = True

    def create_model(self, model_input, vocab_size, num_frames, frame_subset_seed=None, **unused_params):
        num_extend = FLAGS.moe_num_extend
        unused_params.pop("labels", None)
        model_input, num_frames = _random_halves(model_input, num_frames, num_extend, frame_subset_seed)
        result = LstmExtendModel().create_model(model_input, vocab_size, num_frames, **unused_params)
        return {"predictions": _mean_over_replicas(result["predictions"].clamp(0.0, 1.0), num_extend)}


# ---- Z: the LstmMultiscale models -- the scale loop of MultiscaleCnnLstmModel with a learned per-label mix of the scales --------------------
DEFINE_integer("cnn_cells", 256, "Number of CNN cells.")                                             # Z/frame_level_models.py:58


class LstmMultiscaleModel(MultiscaleCnnLstmModel):
    """Z/frame_level_models.py:2827-2986: L = --moe_num_extend scales of MultiscaleCnnLstmModel's loop (_scales) -- einsum CNN with
    256, 256, 512 filters (truncated_normal(stddev=0.1) here), slim.batch_norm over all B F_k rows, ReLU, one BasicLSTMCell inside a
    one-cell MultiRNNCell whose final memory feeds sub_moe, the pair maximum as the next scale's input -- combined per label:
        weight = softmax over the scales of memory_l . ensemble_weight2d[l],   predictions = sum_l weight_l sub_prediction_l
    (ops.scale_mix; the L logit products are one grouped launch each way, ops.linear_group), and
        prediction_frames [B L, V], row b L + l = scale l's sub-prediction for video b,
    which is what Z trains on: train.TrainGraph takes its label loss from prediction_frames and none from predictions (Z/train.py:
    359-379).  predictions_no_grad (TrainGraph.step passes it): predictions is then built without an autograd graph, so no zeros run
    back through the mix and its products; ensemble_weight2d stays a registered Variable under its l2 term.
    Variables: cnn<k>cnn-filter-len{1,2,3}, cnn<k>cluster_bn/{gamma,beta,moving_mean,moving_variance},
    RNN-rnn<k>/multi_rnn_cell/cell_0/basic_lstm_cell/{weights,biases}, gatesmoe<k>/weights, expertsmoe<k>/{weights,biases},
    ensemble_weight2d [L, sum(filters), V] (glorot uniform, l2 1e-8).  The reference multiplies memories --lstm_cells wide by a weight2d
    sum(filters) = 1024 deep: any other --lstm_cells is a shape error there and a ValueError here.
    accepts_quantized_input: as MultiscaleCnnLstmModel."""
    accepts_quantized_input = True
    trains_on_prediction_frames = True       # train.TrainGraph.step: asks for predictions without a graph

    FILTER_INIT = staticmethod(truncated_normal(0.1))
    SCALES_FLAG = "moe_num_extend"
    WEIGHT2D_L2 = 1.0e-8

    def _rnn(self, x_tm, num_frames, d_in, lstm_size, layer):
        g = get_default_graph()
        with g.variable_scope("RNN-rnn%d" % (layer + 1)):
            wb = _lstm_cells(d_in, lstm_size, 1, multi=True)
        _, finals = _native_stack(x_tm, num_frames, wb, slot=layer)
        return finals[0][0]

    def _weight2d_depth(self, features_size, lstm_size):
        if lstm_size != features_size:
            raise ValueError("%s multiplies memories --lstm_cells = %d wide by ensemble_weight2d [L, %d, V], as the reference: "
                             "--lstm_cells must be %d" % (type(self).__name__, lstm_size, features_size, features_size))
        return features_size

    def _weight2d(self, num_extend, vocab_size):
        depth = self._weight2d_depth(sum(self.NUM_FILTERS), int(FLAGS.lstm_cells))
        return get_default_graph().get_variable("ensemble_weight2d", (num_extend, depth, vocab_size), glorot_uniform, l2=self.WEIGHT2D_L2)

    def _combine(self, sub_predictions, memories, weight2d):
        """predictions from the sub-predictions [B,V], the memories [B,H] and ensemble_weight2d."""
        logits = ops.linear_group(memories, [(weight2d, l, None) for l in range(len(memories))])
        return ops.scale_mix(sub_predictions, logits)

    def create_model(self, model_input, vocab_size, num_frames, l2_penalty=1e-8, is_training=True, predictions_no_grad=False,
                     **unused_params):
        num_extend = FLAGS.moe_num_extend
        self._weight2d_depth(sum(self.NUM_FILTERS), int(FLAGS.lstm_cells))                        # refuses before anything is created
        seq_ops.reserve_resident(num_extend, 1)                           # the L stacks are alive in one step
        sub_predictions, memories = self._scales(model_input, vocab_size, num_frames, num_extend, l2_penalty, is_training)
        weight2d = self._weight2d(num_extend, vocab_size)
        if predictions_no_grad:
            with torch.no_grad():
                predictions = self._combine(sub_predictions, memories, weight2d)
        else:
            predictions = self._combine(sub_predictions, memories, weight2d)
        return {"predictions": predictions,
                "prediction_frames": torch.stack(sub_predictions, dim=1).reshape(-1, vocab_size)}


class LstmMultiscale2Model(LstmMultiscaleModel):
    """Z/frame_level_models.py:3160-3373: LstmMultiscaleModel with the scalar-gate cell per scale (_gate_lstm_layer under
    rnn<k>lstm_forward, l2 1e-8, the memory gathered at frame num_frames - 1 of the scale; rows without frames as LstmGateModel) and
    predictions = the plain mean of the sub-predictions (:3372).  ensemble_weight2d and its softmax are built but unused there (:3366-
    3369): the Variable is created (checkpoints carry it; the optimiser moves it by its l2 term alone) and nothing is computed from it.
    Variables: cnn<k>..., rnn<k>lstm_forward/{Wi,Ui,bi,Wf,Uf,bf,Wog,Uog,bog,Wc,Uc,bc}, gatesmoe<k>, expertsmoe<k>, ensemble_weight2d."""

    def _rnn(self, x_tm, num_frames, d_in, lstm_size, layer):
        _, state = _gate_lstm_layer(x_tm, num_frames, lstm_size, "rnn%dlstm_forward" % (layer + 1), 1e-8)     # rnn_gate's own l2_penalty
        return state

    def _combine(self, sub_predictions, memories, weight2d):
        predictions = sub_predictions[0]
        for p in sub_predictions[1:]:
            predictions = predictions + p
        return predictions / float(len(sub_predictions))


class LstmMultiscaleDitillChainModel(LstmMultiscaleModel):
    """Z/frame_level_models.py:2988-3158 (the reference's spelling): LstmMultiscaleModel with filters (c, c, 2 c), c = --cnn_cells, an
    ensemble_weight2d --lstm_cells deep, and a cascade input: each sub_moe reads [memory | relu(FC_256(distillation_predictions))], the FC
    under class_inputsmoe<k> (one per scale, width fixed at 256, l2, NOT l2-normalised; :3051-3059).  The L FCs read one input: they are
    created together before the scale loop and run as one grouped launch each way.  The cascade input arrives as
    distillation_predictions (--distillation_as_input); without it the model is LstmMultiscaleModel with the other widths, as in the
    reference."""
    CLASS_SIZE = 256

    def _weight2d_depth(self, features_size, lstm_size):
        return lstm_size

    def _head_input(self, lstm_memory):
        if self._class_inputs is None:
            return lstm_memory
        return torch.cat([lstm_memory, self._class_inputs[self._scale]], dim=1)

    def create_model(self, model_input, vocab_size, num_frames, distillation_predictions=None, l2_penalty=1e-8, **unused_params):
        c = FLAGS.cnn_cells
        self.NUM_FILTERS = (c, c, 2 * c)
        self._class_inputs = None
        if distillation_predictions is not None:
            g = get_default_graph()
            x = distillation_predictions.to(torch.float32)
            spec = []
            for k in range(FLAGS.moe_num_extend):
                scope = "class_inputsmoe%d" % (k + 1)
                spec.append((g.get_variable(scope + "/weights", (x.shape[1], self.CLASS_SIZE), xavier_uniform, l2=l2_penalty), None,
                             g.get_variable(scope + "/biases", (self.CLASS_SIZE,), zeros)))
            self._class_inputs = [ops.activation(y, "relu") for y in ops.linear_group([x] * len(spec), spec)]
        try:
            return super().create_model(model_input, vocab_size, num_frames, l2_penalty=l2_penalty, **unused_params)
        finally:
            self._class_inputs = None
