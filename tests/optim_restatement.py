"""Plain numpy restatement of the flat-arena optimiser pass (csrc/optim.hip), shared by tests/test_optim_host.py (no GPU) and
tests/test_gpu_optim_branches.py (-m gpu) so that both see identical data.  Nothing here imports torch or the library.

The operation, per tensor t of an arena described by a chunk table (variables.Graph.finalize: every tensor starts on a 64-float
boundary and is cut into chunks of <= 4096 floats):

    ge  = g * gscale + l2[t] * w
    n2[t] = sum ge^2
    cs  = clip / max(sqrt(n2[t]), clip)            (1 when clip <= 0)
    ge  = ge * cs
    m'  = b1 m + (1 - b1) ge
    v'  = b2 v + (1 - b2) ge^2
    w'  = w - lr_t m' / (sqrt(v') + eps)

oracle/np_ref.py (clip_by_norm, adam_step) stays the definition of the algorithm; tests/test_optim_host.py holds `reference` to it.

`reference` evaluates this in float64 from the float32 values the kernel receives: every input AND every hyper-parameter is rounded
to float32 first and then widened (np.float64(np.float32(0.999)), and 1 - that in float64; for b in [0.5, 1] the kernel's own
1.0f - b is exact, so both sides hold the same number).  `restatement_f32` evaluates the same formulas in float32 numpy: it stands for
"a correct fp32 implementation" and must sit well inside the bounds.  VARIANTS are five subtly wrong float64 implementations that
must fall outside them.

Bounds (u = 2^-24, one float32 rounding; K = the number of roundings a path can accumulate, every term at its worst case and all
adding up linearly; hipcc's default sqrtf and division are correctly rounded, a contraction of a product and a sum into an fma only
removes a rounding):

  n2  each ge has 2 roundings (g * gscale; the fma with l2 w), so ge^2 carries 2 * 2 + 1 = 5 (the square itself).  A chunk partial
      is at most 16 serial adds per lane (4 unrolled iterations x (3 adds inside the float4 + 1 accumulate)), a 6-level wave tree
      and 3 adds over the four waves: 25.  The partials are added in float64 and rounded to float32 once: 1.
          K_N = 5 + 25 + 1 = 31, used as 32:            |dn2| <= K_N u n2
      (ge's 2 roundings are relative to |g gscale| + |l2 w|, not to |ge|.  sum |ge| (|g gscale| + |l2 w|) <= sqrt(n2 n2abs) with
      n2abs = sum (|g gscale| + |l2 w|)^2, so the 5 above is 4 sqrt(n2abs / n2) + 1: the case data keep n2abs <= 1.21 n2, asserted in
      tests/test_optim_host.py, which keeps the total at 31.4 <= 32.)
  cs  sqrt halves n2's relative error (16), is rounded (1), and the division is rounded (1):   K_CS = 18
  ge  the 2 roundings above, the product with cs (1) and cs's own error (18):                   K_GE = 21
  m'  (1 - b1) * ge is rounded (1) and carries ge's 21; the fma rounds once more (1), and |m'| <= |b1 m| + |(1 - b1) ge|:
          K_M = 21 + 1 + 1 = 23, used as 24:            |dm| <= K_M u (|b1 m| + |(1 - b1) ge|)
  v'  ((1 - b2) * ge) * ge: two rounded products (2) on ge^2's 2 * 21 = 42, and the fma (1):
          K_V = 42 + 2 + 1 = 45:                        |dv| <= K_V u (|b2 v| + |(1 - b2) ge^2|)
  w'  the step lr_t * m' / (sqrtf(v') + eps): lr_t * m' (1), sqrtf (1) on half of v's 45 (22.5), + eps (1), the division (1), on top of
      m's 24, which is relative to |b1 m| + |(1 - b1) ge| -- m' cancels, so the step is taken at that magnitude; the subtraction from w
      rounds once, relative to |w'|:
          K_W = 24 + 22.5 + 4 = 50.5, used as 51:       |dw| <= u |w'| + K_W u lr_t (|b1 m| + |(1 - b1) ge|) / (sqrt(v') + eps)
      (where m' does not cancel this is the |lr_t m' / (sqrt(v') + eps)| of the plain form; elementwise relative error is useless here:
      a float32 evaluation is 3e4 u off relative to |m'| itself on a million elements and stays at 13 u of |w'| + lr_t.)

The K values come from this count alone; no device output went into them.  yt8m_clip_by_norm_f32 has its own count in `clip_bound`."""
import numpy as np

U = 2.0 ** -24
K_N, K_CS, K_GE, K_M, K_V, K_W = 32.0, 18.0, 21.0, 24.0, 45.0, 51.0
ALIGN, CHUNK = 64, 4096
SENTINEL_BITS = 0x7FC5A5A5          # a quiet NaN with a payload: a padding float that enters any sum or any output shows
# the issue's sixteen tensors and two more, so that the last chunk's length takes every residue modulo 4 (6 and 4098: residue 2)
CHUNK_SIZES = [1, 3, 4, 5, 63, 64, 65, 1021, 1024, 1027, 4095, 4096, 4097, 8192, 12289, 257 * 4096 + 5, 6, 4098]
TILE_SHAPES = [(64, 64), (65, 63), (1000,), (130, 77), (33, 200), (192, 16), (200, 136)]
H2_SHAPES = [(130, 77), (200, 136), (70, 20)]        # the last one is all zeros
CLIP_N = [1, 255, 256, 257, 65539, 4096 * 256 + 7]


def hyper(gscale=0.5, clip=1.0, lr_t=0.01, b1=0.9, b2=0.999, eps=1e-8):
    """The float32 values the kernel receives."""
    return dict(gscale=np.float32(gscale), clip=np.float32(clip), lr_t=np.float32(lr_t), b1=np.float32(b1), b2=np.float32(b2),
                eps=np.float32(eps))


def layout(sizes):
    """Offsets, arena length and chunk table of tensors of `sizes` floats, as variables.Graph.finalize lays them out."""
    offs, chunks, start, off = [], [], [], 0
    for t, n in enumerate(sizes):
        offs.append(off)
        start.append(len(chunks))
        for c0 in range(0, n, CHUNK):
            chunks.append((off + c0, min(CHUNK, n - c0), t, 0))
        off += (n + ALIGN - 1) // ALIGN * ALIGN
    start.append(len(chunks))
    return dict(sizes=[int(n) for n in sizes], offsets=offs, total=off, chunks=np.array(chunks, dtype=np.int32).reshape(-1, 4),
                chunk_start=np.array(start, dtype=np.int32))


def element_maps(case):
    """Per arena element: tensor id (-1 in the padding), chunk id, and whether it lies in its chunk's scalar tail."""
    tid = np.full(case["total"], -1, dtype=np.int64)
    cid = np.full(case["total"], -1, dtype=np.int64)
    tail = np.zeros(case["total"], dtype=bool)
    for c, (x, y, z, _) in enumerate(case["chunks"]):
        tid[x:x + y], cid[x:x + y] = z, c
        tail[x + (y // 4) * 4:x + y] = True
    return tid, cid, tail


def sentinel(n):
    return np.full(n, SENTINEL_BITS, dtype=np.uint32).view(np.float32)


def padding_intact(case, arr):
    tid = element_maps(case)[0]
    return bool((np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32)[tid < 0] == SENTINEL_BITS).all())


# ---- case builders -------------------------------------------------------------------------------------------------------------------
def make_case(shapes, seed, gscale=0.5, name=""):
    """Arenas w, m, v, g (float32, sentinel in the padding) for tensors of `shapes`.  l2 alternates 0 / 1e-3; gradients are
    +-U(0.5, 1.5) scaled per tensor so that |g gscale| is 0.3 (below clip = 1) for tensors 0, 1, 4, 5, ... and 3 (above) for 2, 3, 6, 7, ...;
    weights are U(-5e-3, 5e-3).  Every tensor with more than 4 floats holds cold elements (m = v = 0, |g| in 1e-9 .. 1e-6, |w| <= 1e-4:
    sqrt(v') of the size of eps) and exact-zero elements (g = m = v = 0, and w = 0 where l2 != 0: nothing may move there), none of them
    in the tensor's last four floats, which stay ordinary for the scalar tail.

    Why gradients bounded away from zero and weights this small: the first term of the w bound, u |w'|, is the final rounding of w', and
    a correctly rounded subtraction attains it (w' just above a power of two).  A correct implementation can only stay within HALF of the
    bound where the step term K_W u lr_t (|b1 m| + |(1 - b1) ge|) / (sqrt(v') + eps) is at least as large as u |w'|, element by element:
    |g| >= 0.5 of its scale keeps the step above 1.6e-4 at lr_t = 0.01 (clipped tensors: cs = 1 / 3), 51 times that is 8e-3 >= |w'|.  The
    check loses nothing by it: the bound on w is then ~1e-8 absolute, about what u |w'| alone is for a weight of 0.2."""
    shapes = [tuple(s) if isinstance(s, (tuple, list)) else (int(s),) for s in shapes]
    sizes = [int(np.prod(s)) for s in shapes]
    case = layout(sizes)
    rs = np.random.RandomState(seed)
    w, m, v, g = (sentinel(case["total"]).copy() for _ in range(4))
    l2 = np.array([0.0 if t % 2 == 0 else 1e-3 for t in range(len(sizes))], dtype=np.float32)
    cold, zero = [], []
    for t, n in enumerate(sizes):
        o = case["offsets"][t]
        ratio = 0.3 if (t // 2) % 2 == 0 else 3.0
        gt = rs.choice([-1.0, 1.0], size=n) * rs.uniform(0.5, 1.5, size=n)
        gt *= ratio / (gscale * max(np.sqrt(np.sum(gt * gt)), 1e-30))
        s = ratio / (gscale * np.sqrt(n))                                   # the size of one gradient element
        w[o:o + n] = rs.uniform(-5e-3, 5e-3, size=n).astype(np.float32)
        g[o:o + n] = gt.astype(np.float32)
        m[o:o + n] = (rs.randn(n) * 0.1 * s * gscale).astype(np.float32)
        v[o:o + n] = (rs.uniform(0.25, 1.0, size=n) * (s * gscale) ** 2).astype(np.float32)
        if n > 4:
            for i in [0] + ([n // 2, n // 3] if n >= 16 else []):
                g[o + i] = np.float32(rs.choice([-1.0, 1.0]) * 10.0 ** rs.uniform(-9.0, -6.0))
                w[o + i] = np.float32(rs.uniform(-1e-4, 1e-4))
                m[o + i] = v[o + i] = 0.0
                cold.append(o + i)
            for i in [1] + ([n // 2 + 1] if n >= 16 else []):
                g[o + i] = m[o + i] = v[o + i] = 0.0
                if l2[t] != 0:
                    w[o + i] = 0.0
                zero.append(o + i)
    case.update(name=name, shapes=shapes, w=w, m=m, v=v, g=g, l2=l2, cold=np.array(cold, dtype=np.int64),
                zero=np.array(zero, dtype=np.int64))
    return case


def chunk_case():
    return make_case(CHUNK_SIZES, 11, name="chunk")


def tile_case():
    return make_case(TILE_SHAPES, 12, name="tile")


def h2_case():
    """(130, 77) and (200, 136) with max |w| = 0.9 and empty Adam slots, so that one step at lr_t = 0.2 (every weight moves by about
    0.63) carries max |w| across 1.0; (70, 20) all zeros with zero gradients."""
    case = make_case(H2_SHAPES, 13, name="h2")
    for t in (0, 1):
        o, n = case["offsets"][t], case["sizes"][t]
        case["w"][o:o + n] *= np.float32(0.9) / np.abs(case["w"][o:o + n]).max()
        case["m"][o:o + n] = 0.0
        case["v"][o:o + n] = 0.0
    o, n = case["offsets"][2], case["sizes"][2]
    for k in "wmvg":
        case[k][o:o + n] = 0.0
    case["l2"][:] = 0.0
    return case


def next_step_case(case, w, m, v, seed, gscale=0.5):
    """The same arena one step later: state w, m, v (float32 arenas) and fresh gradients."""
    fresh = make_case(case["shapes"], seed, gscale=gscale, name=case["name"] + "+1")
    out = dict(case)
    out.update(name=fresh["name"], w=np.array(w, dtype=np.float32), m=np.array(m, dtype=np.float32), v=np.array(v, dtype=np.float32),
               g=fresh["g"], cold=np.zeros(0, dtype=np.int64), zero=np.zeros(0, dtype=np.int64))
    return out


def clip_case(n, above):
    """One tensor for yt8m_clip_by_norm_f32 with max_norm = 1: norm 3 (above) or 0.3."""
    rs = np.random.RandomState(1000 + n % 997 + int(above))
    g = rs.randn(n)
    g *= (3.0 if above else 0.3) / np.sqrt(np.sum(g * g))
    return g.astype(np.float32)


# ---- the float64 reference and its wrong variants ------------------------------------------------------------------------------------
def _active(case, tensors, skip):
    on = np.zeros(len(case["sizes"]), dtype=bool)
    for lo, hi in ([(0, len(on))] if tensors is None else tensors):
        on[lo:hi] = True
    if skip is not None:
        on &= ~np.asarray(skip, dtype=bool)
    return on


def reference(case, h, tensors=None, skip=None, variant=None, norms_in=None):
    """float64 evaluation over the tensors of the ranges `tensors` (list of (lo, hi); None = all) that `skip` does not flag.  Returns
    arenas w, m, v (float64; elements outside keep their input), n2 per tensor (outside: norms_in or 0; all zeros when clip <= 0: the
    norm pass does not run), and the magnitudes the bounds need.  skip leaves the norms alone only in the Adam pass: the norm pass
    computes them for every tensor of the ranges, as the device does."""
    f = lambda x: np.float64(np.float32(x))
    gscale, clip, lr, b1, b2, eps = (f(h[k]) for k in ("gscale", "clip", "lr_t", "b1", "b2", "eps"))
    tid, cid, tail = element_maps(case)
    nT = len(case["sizes"])
    in_range = _active(case, tensors, None)
    on = _active(case, tensors, skip)
    idx = np.nonzero((tid >= 0) & in_range[np.maximum(tid, 0)])[0]
    t = tid[idx]
    w, m, v, g = (case[k][idx].astype(np.float64) for k in "wmvg")
    l2 = case["l2"].astype(np.float64)[t]
    ge = g * gscale + l2 * w
    if variant == "gscale_after_l2":
        ge = (g + l2 * w) * gscale
    n2 = np.zeros(nT) if norms_in is None else np.array(norms_in, dtype=np.float64)
    cs = np.ones_like(ge)
    if clip > 0:
        sq = (g * gscale) ** 2 if variant == "norm_without_l2" else ge * ge
        n2t = np.bincount(t, weights=sq, minlength=nT)
        n2[in_range] = n2t[in_range]
        if variant == "norm_per_chunk":
            n2c = np.bincount(cid[idx], weights=sq, minlength=len(case["chunks"]))
            cs = clip / np.maximum(np.sqrt(n2c[cid[idx]]), clip)
        else:
            cs = clip / np.maximum(np.sqrt(n2t[t]), clip)
    ge = ge * cs
    mag_m = np.abs(b1 * m) + np.abs((1.0 - b1) * ge)
    mag_v = np.abs(b2 * v) + np.abs((1.0 - b2) * ge * ge)
    m1 = b1 * m + (1.0 - b1) * ge
    v1 = b2 * v + (1.0 - b2) * ge * ge
    den = np.sqrt(v1 + eps) if variant == "eps_in_root" else np.sqrt(v1) + eps
    w1 = w - lr * m1 / den
    mag_w = lr * mag_m / (np.sqrt(v1) + eps)
    keep = ~on[t]
    if variant == "tail_untouched":
        keep = keep | tail[idx]
    m1[keep], v1[keep], w1[keep] = m[keep], v[keep], w[keep]
    out = dict(n2=n2, idx=idx, updated=idx[~keep])
    for k, val, mag in (("w", w1, mag_w), ("m", m1, mag_m), ("v", v1, mag_v)):
        full = case[k].astype(np.float64)
        full[idx] = val
        out[k] = full
        fm = np.zeros(case["total"])
        fm[idx] = np.where(keep, 0.0, mag)
        out["mag_" + k] = fm
    return out


VARIANTS = ["eps_in_root", "norm_without_l2", "norm_per_chunk", "gscale_after_l2", "tail_untouched"]


def n2_abs(case, h):
    """sum (|g gscale| + |l2 w|)^2 per tensor: what the two roundings of ge are relative to (see the derivation of K_N)."""
    tid = element_maps(case)[0]
    idx = np.nonzero(tid >= 0)[0]
    a = np.abs(case["g"][idx].astype(np.float64) * np.float64(h["gscale"])) + \
        np.abs(case["l2"].astype(np.float64)[tid[idx]] * case["w"][idx].astype(np.float64))
    return np.bincount(tid[idx], weights=a * a, minlength=len(case["sizes"]))


def bounds(ref):
    """Absolute bounds on n2 (per tensor) and on the arenas m, v, w (0 where nothing may change: those must be exact)."""
    return dict(n2=K_N * U * ref["n2"], m=K_M * U * ref["mag_m"], v=K_V * U * ref["mag_v"],
                w=np.where(ref["mag_m"] > 0, U * np.abs(ref["w"]), 0.0) + K_W * U * ref["mag_w"])


def worst_ratio(got, want, bound):
    """max |got - want| / bound; an error where the bound is 0 is infinite."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def ratios(ref, n2, w, m, v, tensors=None):
    """{output: worst error / bound} of a result (float32 arenas and per-tensor norms) over the elements the reference updated."""
    b = bounds(ref)
    i = ref["updated"]
    on = _active(dict(sizes=ref["n2"]), tensors, None)
    out = dict((k, worst_ratio(arr[i], ref[k][i], b[k][i])) for k, arr in (("m", m), ("v", v), ("w", w)))
    out["norms"] = 0.0 if n2 is None else worst_ratio(np.asarray(n2, dtype=np.float64)[on], ref["n2"][on], b["n2"][on])
    return out


# ---- "a correct fp32 implementation" -------------------------------------------------------------------------------------------------
def restatement_f32(case, h, tensors=None, skip=None):
    """The same formulas in float32 numpy (products and sums rounded one by one; chunk partials summed in float32, the partials of a
    tensor in float64 and rounded once, as the device does).  Returns n2 (float32 per tensor) and the arenas w, m, v."""
    one = np.float32(1.0)
    gscale, clip, lr, b1, b2, eps = (np.float32(h[k]) for k in ("gscale", "clip", "lr_t", "b1", "b2", "eps"))
    tid = element_maps(case)[0]
    nT = len(case["sizes"])
    in_range = _active(case, tensors, None)
    on = _active(case, tensors, skip)
    w, m, v = case["w"].copy(), case["m"].copy(), case["v"].copy()
    n2 = np.zeros(nT, dtype=np.float32)
    if clip > 0:
        part = np.zeros(len(case["chunks"]))
        for c, (x, y, z, _) in enumerate(case["chunks"]):
            if in_range[z]:
                ge = case["g"][x:x + y] * gscale + case["l2"][z] * case["w"][x:x + y]
                part[c] = np.sum(ge * ge, dtype=np.float32)
        for t in range(nT):
            if in_range[t]:
                n2[t] = np.float32(part[case["chunk_start"][t]:case["chunk_start"][t + 1]].sum())
    for t in range(nT):
        if not on[t]:
            continue
        o, n = case["offsets"][t], case["sizes"][t]
        cs = clip / np.maximum(np.sqrt(n2[t]), clip) if clip > 0 else one
        ge = (case["g"][o:o + n] * gscale + case["l2"][t] * case["w"][o:o + n]) * np.float32(cs)
        m[o:o + n] = b1 * case["m"][o:o + n] + (one - b1) * ge
        v[o:o + n] = b2 * case["v"][o:o + n] + (one - b2) * ge * ge
        w[o:o + n] = case["w"][o:o + n] - lr * m[o:o + n] / (np.sqrt(v[o:o + n]) + eps)
    assert w.dtype == m.dtype == v.dtype == np.float32
    return n2, w, m, v


# ---- yt8m_clip_by_norm_f32 -----------------------------------------------------------------------------------------------------------
def clip_reference(g, max_norm):
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    mx = np.float64(np.float32(max_norm))
    return g * (mx / max(np.sqrt(np.sum(g * g)), mx))


def clip_bound(g, max_norm):
    """|d out| <= K u |out|: each square is rounded (1); a lane adds ceil(n / 65536) of them serially (256 workgroups of 256 lanes),
    then a 6-level wave tree and 3 adds (9); every workgroup of the second kernel adds the 256 partials the same way (9).  The factor
    max_norm / max(sqrt(tot), max_norm): half of that sum, sqrtf (1) and the division (1); the product with g (1)."""
    n = len(g)
    k_sum = 1 + (n + 65535) // 65536 + 9 + 9
    return (k_sum / 2.0 + 3.0) * U * np.abs(clip_reference(g, max_norm))


# ---- the cases of tests/test_gpu_optim_branches.py, as data (the second steps start from restatement_f32's state here, from the
# device's own state there) -------------------------------------------------------------------------------------------------------------
SUB_RANGE = (5, 13)
SKIP_TENSORS = (3, 8, 15)
TWO_RANGES = [(0, 5), (7, 7), (9, len(CHUNK_SIZES))]
H2_LR = (0.001, 0.2, 0.001)


def skip_mask(n, flagged=SKIP_TENSORS):
    s = np.zeros(n, dtype=np.uint8)
    s[list(flagged)] = 1
    return s


def host_cases():
    """(name, case, hyper, tensor ranges or None, skip mask or None) for every arena the GPU module runs."""
    c, t, q = chunk_case(), tile_case(), h2_case()
    out = [("chunk-clip1", c, hyper(), None, None), ("chunk-clip0", c, hyper(clip=0.0), None, None),
           ("chunk-range", c, hyper(), [SUB_RANGE], None), ("chunk-skip", c, hyper(), None, skip_mask(len(CHUNK_SIZES))),
           ("chunk-two-ranges", c, hyper(), TWO_RANGES, None)]
    _, w, m, v = restatement_f32(c, hyper())
    out.append(("chunk-step2", next_step_case(c, w, m, v, 21), hyper(lr_t=0.02), None, None))
    out.append(("tile", t, hyper(), None, None))
    _, w, m, v = restatement_f32(t, hyper())
    out.append(("tile-range", next_step_case(t, w, m, v, 22), hyper(), [(3, 6)], None))
    for i, lr in enumerate(H2_LR):
        out.append(("h2-step%d" % (i + 1), q, hyper(lr_t=lr), None, None))
        _, w, m, v = restatement_f32(q, hyper(lr_t=lr))
        q = next_step_case(q, w, m, v, 30 + i)
        o, n = q["offsets"][2], q["sizes"][2]
        q["g"][o:o + n] = 0.0                                                # the all-zero matrix keeps zero gradients
    return out
