"""The launch plans of the persistent recurrences (youtube-8m_amd/csrc/persist_plan.h) as a literal table, checked without a GPU.

tests/persist_plan_main.cpp includes the header, is built with the host C++ compiler and prints the plan of every case it reads.  A
case is `direction cus cap_fwd cap_bwd tape_mode B H T workspace_bytes product images maxima gru [knob=value ...]` (product 0 fp32,
1 bf16, 2 h2; knobs by their PersistKnobs field names, defaults otherwise).  The expected line is
  forward : code ok geo=NQ,NU,RB,NT16,per,pf grid nimg form pack SH PD NKB | q=supported,gru_supported,fwd_on_bf16_pipe
            sizes=workspace_bytes,workspace_bytes_steps(T),gru_workspace_bytes(T) | refusal message
  backward: code ok geo grid nimg form SH PF ROT TPF sc=offset,bytes | q=bwd_supported,bwd_on_f16_pipe,bwd_images_rows
            steps=workspace_bytes_steps(T) | message
(a refused plan prints no launch fields).  The q fields are what the (B, H) query entry points answer on that device and caps.

The expected values were derived from the code this header replaced -- persist_geometry, persist_geometry_bwd, fwd_x3_shape, bwd_rot,
launch_bwd_sh and the two *_impl functions of lstm_persist.hip -- not from the header's output.  One answer differs from that code on
purpose: yt8m_lstm_persist_bwd_on_f16_pipe ignored YT8M_PERSIST_BWD_H2=0, which the launch and include/yt8m_hip.h honour; read from
the plan it is 0 there (the bwd_h2=0 row).

GPU_TABLE holds the launches tests/test_gpu_persist_forms.py makes on a 256-CU device; tests/golden/persist_forms_seen.txt is the
list of kernel instantiations a profiled run of that file showed (tools/persist_forms_list.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = [
    # support edges: B = 0 and 1, the H ladders of both directions
    ("fwd 256 -1 -1 0 0 1024 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 sizes=0,0,0 | shape not supported by the persistent recurrence (see yt8m_lstm_persist_supported)"),
    ("fwd 256 -1 -1 0 1 1024 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,1,8,0 grid=128 nimg=1048576 form=fp32 pack=plain SH=1 PD=0 NKB=0 | q=1,1,0 sizes=591104,1381632,1049856 | "),
    ("bwd 256 -1 -1 0 0 1024 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 steps=0 | shape not supported by the persistent backward recurrence (see yt8m_lstm_persist_bwd_supported)"),
    ("bwd 256 -1 -1 0 1 1024 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=32,64,1,1,8,0 grid=64 nimg=1048576 form=fp32 SH=1 PF=0 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=1381632 | "),
    ("fwd 256 -1 -1 0 64 127 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 sizes=0,0,0 | shape not supported by the persistent recurrence (see yt8m_lstm_persist_supported)"),
    ("fwd 256 -1 -1 0 64 128 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=1,16,1,4,8,1 grid=16 nimg=1048576 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,0,0 sizes=332032,727296,561408 | "),
    ("fwd 256 -1 -1 0 64 256 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=2,32,1,4,8,1 grid=32 nimg=1048576 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=594176,1384704,1052928 | "),
    ("fwd 256 -1 -1 0 64 384 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 sizes=0,0,0 | shape not supported by the persistent recurrence (see yt8m_lstm_persist_supported)"),
    ("fwd 256 -1 -1 0 64 512 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=4,64,1,4,8,1 grid=64 nimg=1048576 form=x3_six pack=x3_three SH=1 PD=1 NKB=2 | q=1,1,1 sizes=1118464,2699520,2035968 | "),
    ("fwd 256 -1 -1 0 64 768 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=6,96,1,4,8,1 grid=96 nimg=1048576 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=1642752,4014336,3019008 | "),
    ("fwd 256 -1 -1 0 64 1024 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,4,8,1 grid=128 nimg=1048576 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=2167040,5329152,4002048 | "),
    ("fwd 256 -1 -1 0 64 1152 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 sizes=0,0,0 | shape not supported by the persistent recurrence (see yt8m_lstm_persist_supported)"),
    ("bwd 256 -1 -1 0 64 128 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=4,8,2,4,4,1 grid=16 nimg=1048576 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=727296 | "),
    ("bwd 256 -1 -1 0 64 192 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 steps=0 | shape not supported by the persistent backward recurrence (see yt8m_lstm_persist_bwd_supported)"),
    ("bwd 256 -1 -1 0 64 256 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=8,16,2,4,4,1 grid=32 nimg=1048576 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=1384704 | "),
    ("bwd 256 -1 -1 0 64 512 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=16,32,2,4,4,1 grid=64 nimg=1048576 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=2699520 | "),
    ("bwd 256 -1 -1 0 64 768 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=24,48,2,4,4,1 grid=96 nimg=1048576 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=4014336 | "),
    ("bwd 256 -1 -1 0 64 1024 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=1048576 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    # support edges: cus one below NU (forward NU = H / 8; the backward needs the forward's support too), and at NU
    ("fwd 127 -1 -1 0 128 1024 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 sizes=0,0,0 | shape not supported by the persistent recurrence (see yt8m_lstm_persist_supported)"),
    ("bwd 127 -1 -1 0 128 1024 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 steps=0 | shape not supported by the persistent backward recurrence (see yt8m_lstm_persist_bwd_supported)"),
    ("fwd 128 -1 -1 0 128 1024 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,8,8,2 grid=128 nimg=1048576 form=x3_six pack=x3_three SH=1 PD=2 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 128 -1 -1 0 128 1024 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=1048576 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("fwd 63 -1 -1 0 128 512 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 sizes=0,0,0 | shape not supported by the persistent recurrence (see yt8m_lstm_persist_supported)"),
    ("bwd 63 -1 -1 0 128 512 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 steps=0 | shape not supported by the persistent backward recurrence (see yt8m_lstm_persist_bwd_supported)"),
    ("fwd 64 -1 -1 0 128 512 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=4,64,1,8,8,2 grid=64 nimg=1048576 form=x3_six pack=x3_three SH=1 PD=2 NKB=2 | q=1,1,1 sizes=2171136,5333248,4006144 | "),
    ("bwd 64 -1 -1 0 128 512 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=16,32,2,8,4,1 grid=64 nimg=1048576 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=5333248 | "),
    # support edges: a batch one tile past MAX_LOCAL_TILES x RB (64 x 2 tiles at H = 1024 on 256 CUs; 64 x 1 under the forward cap of 128)
    ("fwd 256 -1 -1 0 2048 1024 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,128,4,2 grid=256 nimg=1048576 form=x3_six pack=x3_three SH=1 PD=2 NKB=4 | q=1,1,1 sizes=67305728,168493312,126025984 | "),
    ("bwd 256 -1 -1 0 2048 1024 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,128,4,1 grid=128 nimg=1048576 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=168493312 | "),
    ("fwd 256 -1 -1 0 2049 1024 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 sizes=0,0,0 | shape not supported by the persistent recurrence (see yt8m_lstm_persist_supported)"),
    ("bwd 256 -1 -1 0 2049 1024 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 steps=0 | shape not supported by the persistent backward recurrence (see yt8m_lstm_persist_bwd_supported)"),
    ("fwd 256 128 -1 0 1024 1024 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,64,8,2 grid=128 nimg=1048576 form=x3_six pack=x3_three SH=1 PD=2 NKB=4 | q=1,1,1 sizes=33685760,84279552,63045888 | "),
    ("bwd 256 128 -1 0 1024 1024 4 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,64,4,1 grid=128 nimg=1048576 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=84279552 | "),
    ("fwd 256 128 -1 0 1025 1024 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 sizes=0,0,0 | shape not supported by the persistent recurrence (see yt8m_lstm_persist_supported)"),
    ("bwd 256 128 -1 0 1025 1024 4 1152921504606846976 0 0 0 0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 steps=0 | shape not supported by the persistent backward recurrence (see yt8m_lstm_persist_bwd_supported)"),
    # geometry at 256 CUs, default caps, on the per-step workspace of T = 4
    ("fwd 256 -1 -1 0 16 128 4 231168 0 0 0 0",
     "code=0 ok=1 geo=1,16,1,1,8,0 grid=16 nimg=20 form=fp32 pack=plain SH=1 PD=0 NKB=0 | q=1,0,0 sizes=132352,231168,189696 | "),
    ("bwd 256 -1 -1 0 16 128 4 231168 0 0 0 0",
     "code=0 ok=1 geo=4,8,1,1,8,0 grid=8 nimg=5 form=fp32 SH=1 PF=0 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=231168 | "),
    ("fwd 256 -1 -1 0 64 1024 4 5329152 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,4,8,1 grid=128 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=2167040,5329152,4002048 | "),
    ("bwd 256 -1 -1 0 64 1024 4 5329152 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    ("fwd 256 -1 -1 0 128 512 4 5333248 0 0 0 0",
     "code=0 ok=1 geo=4,64,2,8,4,1 grid=128 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=2 | q=1,1,1 sizes=2171136,5333248,4006144 | "),
    ("bwd 256 -1 -1 0 128 512 4 5333248 0 0 0 0",
     "code=0 ok=1 geo=16,32,4,8,2,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5333248 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("fwd 256 -1 -1 0 256 768 4 15859968 0 0 0 0",
     "code=0 ok=1 geo=6,96,2,16,4,2 grid=192 nimg=20 form=fp32 pack=plain SH=1 PD=2 NKB=0 | q=1,1,0 sizes=6373632,15859968,11878656 | "),
    ("bwd 256 -1 -1 0 256 768 4 15859968 0 0 0 0",
     "code=0 ok=1 geo=24,48,2,16,4,1 grid=96 nimg=5 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,0,8 steps=15859968 | "),
    ("fwd 256 -1 -1 0 1024 1024 4 84279552 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,64,4,2 grid=256 nimg=20 form=x3_six pack=x3_three SH=1 PD=2 NKB=4 | q=1,1,1 sizes=33685760,84279552,63045888 | "),
    ("bwd 256 -1 -1 0 1024 1024 4 84279552 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,64,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=84279552 | "),
    # the same with the forward cap at 128 (what CapGuard and bidirectional_lstm_stacks set)
    ("fwd 256 128 -1 0 16 128 4 231168 0 0 0 0",
     "code=0 ok=1 geo=1,16,1,1,8,0 grid=16 nimg=20 form=fp32 pack=plain SH=1 PD=0 NKB=0 | q=1,0,0 sizes=132352,231168,189696 | "),
    ("bwd 256 128 -1 0 16 128 4 231168 0 0 0 0",
     "code=0 ok=1 geo=4,8,1,1,8,0 grid=8 nimg=5 form=fp32 SH=1 PF=0 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=231168 | "),
    ("fwd 256 128 -1 0 64 1024 4 5329152 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,4,8,1 grid=128 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=2167040,5329152,4002048 | "),
    ("bwd 256 128 -1 0 64 1024 4 5329152 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    ("fwd 256 128 -1 0 128 512 4 5333248 0 0 0 0",
     "code=0 ok=1 geo=4,64,2,8,4,1 grid=128 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=2 | q=1,1,1 sizes=2171136,5333248,4006144 | "),
    ("bwd 256 128 -1 0 128 512 4 5333248 0 0 0 0",
     "code=0 ok=1 geo=16,32,4,8,2,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5333248 | "),
    ("fwd 256 128 -1 0 128 1024 4 10592512 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,8,8,2 grid=128 nimg=20 form=x3_six pack=x3_three SH=1 PD=2 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 128 -1 0 128 1024 4 10592512 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("fwd 256 128 -1 0 256 768 4 15859968 0 0 0 0",
     "code=0 ok=1 geo=6,96,1,16,8,2 grid=96 nimg=20 form=fp32 pack=plain SH=1 PD=2 NKB=0 | q=1,1,0 sizes=6373632,15859968,11878656 | "),
    ("bwd 256 128 -1 0 256 768 4 15859968 0 0 0 0",
     "code=0 ok=1 geo=24,48,2,16,4,1 grid=96 nimg=5 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,0,8 steps=15859968 | "),
    ("fwd 256 128 -1 0 1024 1024 4 84279552 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,64,8,2 grid=128 nimg=20 form=x3_six pack=x3_three SH=1 PD=2 NKB=4 | q=1,1,1 sizes=33685760,84279552,63045888 | "),
    ("bwd 256 128 -1 0 1024 1024 4 84279552 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,64,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=84279552 | "),
    # PD edges: nit_min 1 / 2 / 7 / 8 forward (H = 1024: B = 16, 32, 112 and 224, 256), PF edge 1 / 2 backward; ROT edge NT16 % (4 RB) (B = 100: 7 tiles)
    ("fwd 256 -1 -1 0 16 1024 4 1381632 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,1,8,0 grid=128 nimg=20 form=fp32 pack=plain SH=1 PD=0 NKB=0 | q=1,1,0 sizes=591104,1381632,1049856 | "),
    ("fwd 256 -1 -1 0 32 1024 4 2697472 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,2,8,1 grid=128 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=1116416,2697472,2033920 | "),
    ("fwd 256 -1 -1 0 112 1024 4 9276672 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,7,8,1 grid=128 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=3742976,9276672,6954240 | "),
    ("fwd 256 -1 -1 0 224 1024 4 18487552 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,14,4,1 grid=256 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=7420160,18487552,13842688 | "),
    ("fwd 256 -1 -1 0 256 1024 4 21119232 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,16,4,2 grid=256 nimg=20 form=x3_six pack=x3_three SH=1 PD=2 NKB=4 | q=1,1,1 sizes=8470784,21119232,15810816 | "),
    ("bwd 256 -1 -1 0 16 1024 4 1381632 2 0 0 0",
     "code=0 ok=1 geo=32,64,1,1,8,0 grid=64 nimg=5 form=fp32 SH=1 PF=0 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=1381632 | "),
    ("bwd 256 -1 -1 0 32 1024 4 2697472 2 0 0 0",
     "code=0 ok=1 geo=32,64,1,2,8,1 grid=64 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=2697472 | "),
    ("bwd 256 -1 -1 0 100 1024 4 9276672 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,7,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=9276672 | "),
    # workspace edges, forward at (128, 1024): the minimum, the per-step size, room for T images of 1x and of 1.5x width; one byte less than each; T = 1
    ("fwd 256 -1 -1 0 128 1024 4 4268288 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=8 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("fwd 256 -1 -1 0 128 1024 4 4268287 0 0 0 0",
     "code=-2 ok=1 geo=8,128,2,8,4,1 grid=256 | q=1,1,1 sizes=4268288,10592512,7938304 | workspace too small"),
    ("fwd 256 -1 -1 0 128 1024 12 27435264 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=52 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,27435264,20521216 | "),
    ("fwd 256 -1 -1 0 128 1024 12 27435263 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=52 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,27435264,20521216 | "),
    ("fwd 256 -1 -1 0 128 1024 12 6365440 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=12 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,1 sizes=4268288,27435264,20521216 | "),
    ("fwd 256 -1 -1 0 128 1024 12 6365439 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=11 form=fp32 pack=plain SH=0 PD=1 NKB=0 | q=1,1,1 sizes=4268288,27435264,20521216 | "),
    ("fwd 256 -1 -1 0 128 1024 12 9511168 2 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=18 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,27435264,20521216 | "),
    ("fwd 256 -1 -1 0 128 1024 12 9511167 2 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=17 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,1 sizes=4268288,27435264,20521216 | "),
    ("fwd 256 -1 -1 0 128 1024 1 6381824 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=12 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,6381824,3219712 | "),
    ("fwd 256 -1 -1 0 128 1024 1 6381824 2 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=12 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,6381824,3219712 | "),
    ("fwd 256 -1 -1 0 128 1024 1048576 1152921504606846976 0 0 0 0",
     "code=-2 ok=1 geo=8,128,2,8,4,1 grid=256 | q=1,1,1 sizes=4268288,2207615361280,1649269088512 | T too large"),
    ("fwd 256 -1 -1 0 128 1024 1048575 1152921504606846976 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=1048576 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,2207613255936,1649267515648 | "),
    # workspace edges, backward at (128, 1024): the minimum, the per-step size, room for T images, for T images + the h2 scale words; one byte less; T = 1
    ("bwd 256 -1 -1 0 128 1024 4 4268288 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=2 form=fp32 SH=0 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 4268287 2 0 0 0",
     "code=-2 ok=1 geo=32,64,2,8,4,1 grid=128 | q=1,1,8 steps=10592512 | workspace too small"),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592511 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494207,32768 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 8462592 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=4 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 8462591 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=3 form=fp32 SH=0 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 8495360 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=4 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=8397056,32768 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 8495359 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=4 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 1 6381824 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=3 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=6308096,8192 | q=1,1,8 steps=6381824 | "),
    ("bwd 256 -1 -1 0 128 1024 1048576 1152921504606846976 0 0 0 0",
     "code=-2 ok=1 geo=32,64,2,8,4,1 grid=128 | q=1,1,8 steps=2207615361280 | T too large"),
    ("bwd 256 -1 -1 0 128 1024 1048575 1152921504606846976 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=1048576 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=2207613255936 | "),
    # every request against every shape class, forward (per-step workspace, T = 4): fp32 / bf16 / h2
    ("fwd 256 -1 -1 0 16 128 4 231168 1 0 0 0",
     "code=0 ok=1 geo=1,16,1,1,8,0 grid=16 nimg=20 form=fp32 pack=plain SH=1 PD=0 NKB=0 | q=1,0,0 sizes=132352,231168,189696 | "),
    ("fwd 256 -1 -1 0 16 128 4 231168 2 0 0 0",
     "code=0 ok=1 geo=1,16,1,1,8,0 grid=16 nimg=20 form=fp32 pack=plain SH=1 PD=0 NKB=0 | q=1,0,0 sizes=132352,231168,189696 | "),
    ("fwd 256 -1 -1 0 32 256 4 725248 0 0 0 0",
     "code=0 ok=1 geo=2,32,1,2,8,1 grid=32 nimg=20 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=329984,725248,559360 | "),
    ("fwd 256 -1 -1 0 32 256 4 725248 1 0 0 0",
     "code=0 ok=1 geo=2,32,1,2,8,1 grid=32 nimg=20 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=329984,725248,559360 | "),
    ("fwd 256 -1 -1 0 32 256 4 725248 2 0 0 0",
     "code=0 ok=1 geo=2,32,1,2,8,1 grid=32 nimg=20 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=329984,725248,559360 | "),
    ("fwd 256 -1 -1 0 48 768 4 3027200 0 0 0 0",
     "code=0 ok=1 geo=6,96,1,3,8,1 grid=96 nimg=20 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=1248512,3027200,2280704 | "),
    ("fwd 256 -1 -1 0 48 768 4 3027200 1 0 0 0",
     "code=0 ok=1 geo=6,96,1,3,8,1 grid=96 nimg=20 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=1248512,3027200,2280704 | "),
    ("fwd 256 -1 -1 0 48 768 4 3027200 2 0 0 0",
     "code=0 ok=1 geo=6,96,1,3,8,1 grid=96 nimg=20 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=1248512,3027200,2280704 | "),
    ("fwd 256 -1 -1 0 64 1024 4 5329152 1 0 0 0",
     "code=0 ok=1 geo=8,128,1,4,8,1 grid=128 nimg=20 form=bf16_one_plane pack=x3_one SH=1 PD=1 NKB=4 | q=1,1,1 sizes=2167040,5329152,4002048 | "),
    ("fwd 256 -1 -1 0 64 1024 4 5329152 2 0 0 0",
     "code=0 ok=1 geo=8,128,1,4,8,1 grid=128 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=2167040,5329152,4002048 | "),
    ("fwd 256 -1 -1 0 128 512 4 5333248 1 0 0 0",
     "code=0 ok=1 geo=4,64,2,8,4,1 grid=128 nimg=20 form=bf16_one_plane pack=x3_one SH=1 PD=1 NKB=2 | q=1,1,1 sizes=2171136,5333248,4006144 | "),
    ("fwd 256 -1 -1 0 128 512 4 5333248 2 0 0 0",
     "code=0 ok=1 geo=4,64,2,8,4,1 grid=128 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=2 | q=1,1,1 sizes=2171136,5333248,4006144 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 1 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=bf16_one_plane pack=x3_one SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    # ... backward: fp32 / bf16 / h2, images (alone and with bf16: images win), maxima (alone and with h2)
    ("bwd 256 -1 -1 0 16 128 4 231168 1 0 0 0",
     "code=0 ok=1 geo=4,8,1,1,8,0 grid=8 nimg=5 form=fp32 SH=1 PF=0 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=231168 | "),
    ("bwd 256 -1 -1 0 16 128 4 231168 2 0 0 0",
     "code=0 ok=1 geo=4,8,1,1,8,0 grid=8 nimg=5 form=fp32 SH=1 PF=0 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=231168 | "),
    ("bwd 256 -1 -1 0 16 128 4 231168 0 1 0 0",
     "code=-2 ok=1 geo=4,8,1,1,8,0 grid=8 | q=1,0,0 steps=231168 | operand images need the rotated backward epilogue"),
    ("bwd 256 -1 -1 0 16 128 4 231168 1 1 0 0",
     "code=-2 ok=1 geo=4,8,1,1,8,0 grid=8 | q=1,0,0 steps=231168 | operand images need the rotated backward epilogue"),
    ("bwd 256 -1 -1 0 16 128 4 231168 0 0 1 0",
     "code=-2 ok=1 geo=4,8,1,1,8,0 grid=8 | q=1,0,0 steps=231168 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    ("bwd 256 -1 -1 0 16 128 4 231168 2 0 1 0",
     "code=-2 ok=1 geo=4,8,1,1,8,0 grid=8 | q=1,0,0 steps=231168 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    ("bwd 256 -1 -1 0 32 256 4 725248 0 0 0 0",
     "code=0 ok=1 geo=8,16,1,2,8,1 grid=16 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=725248 | "),
    ("bwd 256 -1 -1 0 32 256 4 725248 1 0 0 0",
     "code=0 ok=1 geo=8,16,1,2,8,1 grid=16 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=725248 | "),
    ("bwd 256 -1 -1 0 32 256 4 725248 2 0 0 0",
     "code=0 ok=1 geo=8,16,1,2,8,1 grid=16 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=725248 | "),
    ("bwd 256 -1 -1 0 32 256 4 725248 0 1 0 0",
     "code=-2 ok=1 geo=8,16,1,2,8,1 grid=16 | q=1,0,0 steps=725248 | operand images need the rotated backward epilogue"),
    ("bwd 256 -1 -1 0 32 256 4 725248 1 1 0 0",
     "code=-2 ok=1 geo=8,16,1,2,8,1 grid=16 | q=1,0,0 steps=725248 | operand images need the rotated backward epilogue"),
    ("bwd 256 -1 -1 0 32 256 4 725248 0 0 1 0",
     "code=-2 ok=1 geo=8,16,1,2,8,1 grid=16 | q=1,0,0 steps=725248 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    ("bwd 256 -1 -1 0 32 256 4 725248 2 0 1 0",
     "code=-2 ok=1 geo=8,16,1,2,8,1 grid=16 | q=1,0,0 steps=725248 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    ("bwd 256 -1 -1 0 48 768 4 3027200 0 0 0 0",
     "code=0 ok=1 geo=24,48,1,3,8,1 grid=48 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=3027200 | "),
    ("bwd 256 -1 -1 0 48 768 4 3027200 1 0 0 0",
     "code=0 ok=1 geo=24,48,1,3,8,1 grid=48 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=3027200 | "),
    ("bwd 256 -1 -1 0 48 768 4 3027200 2 0 0 0",
     "code=0 ok=1 geo=24,48,1,3,8,1 grid=48 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=3027200 | "),
    ("bwd 256 -1 -1 0 48 768 4 3027200 0 1 0 0",
     "code=-2 ok=1 geo=24,48,1,3,8,1 grid=48 | q=1,0,0 steps=3027200 | operand images need the rotated backward epilogue"),
    ("bwd 256 -1 -1 0 48 768 4 3027200 1 1 0 0",
     "code=-2 ok=1 geo=24,48,1,3,8,1 grid=48 | q=1,0,0 steps=3027200 | operand images need the rotated backward epilogue"),
    ("bwd 256 -1 -1 0 48 768 4 3027200 0 0 1 0",
     "code=-2 ok=1 geo=24,48,1,3,8,1 grid=48 | q=1,0,0 steps=3027200 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    ("bwd 256 -1 -1 0 48 768 4 3027200 2 0 1 0",
     "code=-2 ok=1 geo=24,48,1,3,8,1 grid=48 | q=1,0,0 steps=3027200 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    ("bwd 256 -1 -1 0 64 1024 4 5329152 1 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    ("bwd 256 -1 -1 0 64 1024 4 5329152 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    ("bwd 256 -1 -1 0 64 1024 4 5329152 0 1 0 0",
     "code=-2 ok=1 geo=32,64,2,4,4,1 grid=128 | q=1,0,0 steps=5329152 | operand images need the rotated backward epilogue"),
    ("bwd 256 -1 -1 0 64 1024 4 5329152 1 1 0 0",
     "code=-2 ok=1 geo=32,64,2,4,4,1 grid=128 | q=1,0,0 steps=5329152 | operand images need the rotated backward epilogue"),
    ("bwd 256 -1 -1 0 64 1024 4 5329152 0 0 1 0",
     "code=-2 ok=1 geo=32,64,2,4,4,1 grid=128 | q=1,0,0 steps=5329152 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    ("bwd 256 -1 -1 0 64 1024 4 5329152 2 0 1 0",
     "code=-2 ok=1 geo=32,64,2,4,4,1 grid=128 | q=1,0,0 steps=5329152 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    ("bwd 256 -1 -1 0 128 512 4 5333248 1 0 0 0",
     "code=0 ok=1 geo=16,32,4,8,2,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5333248 | "),
    ("bwd 256 -1 -1 0 128 512 4 5333248 2 0 0 0",
     "code=0 ok=1 geo=16,32,4,8,2,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5333248 | "),
    ("bwd 256 -1 -1 0 128 512 4 5333248 0 1 0 0",
     "code=-2 ok=1 geo=16,32,4,8,2,1 grid=128 | q=1,0,0 steps=5333248 | operand images need the rotated backward epilogue"),
    ("bwd 256 -1 -1 0 128 512 4 5333248 1 1 0 0",
     "code=-2 ok=1 geo=16,32,4,8,2,1 grid=128 | q=1,0,0 steps=5333248 | operand images need the rotated backward epilogue"),
    ("bwd 256 -1 -1 0 128 512 4 5333248 0 0 1 0",
     "code=-2 ok=1 geo=16,32,4,8,2,1 grid=128 | q=1,0,0 steps=5333248 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    ("bwd 256 -1 -1 0 128 512 4 5333248 2 0 1 0",
     "code=-2 ok=1 geo=16,32,4,8,2,1 grid=128 | q=1,0,0 steps=5333248 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 1 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=bf16 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 0 1 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=images SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 1 1 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=images SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 0 0 1 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 1 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    # images and maxima on the two-image workspace (no SH), images with maxima
    ("bwd 256 -1 -1 0 128 1024 4 4268288 0 1 0 0",
     "code=-2 ok=1 geo=32,64,2,8,4,1 grid=128 | q=1,1,8 steps=10592512 | operand images need one exchange image per step"),
    ("bwd 256 -1 -1 0 128 1024 4 4268288 0 0 1 0",
     "code=-2 ok=1 geo=32,64,2,8,4,1 grid=128 | q=1,1,8 steps=10592512 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    ("bwd 256 -1 -1 0 64 1024 4 2167040 0 1 0 0",
     "code=-2 ok=1 geo=32,64,2,4,4,1 grid=128 | q=1,0,0 steps=5329152 | operand images need one exchange image per step"),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 0 1 1 0",
     "code=-2 ok=1 geo=32,64,2,8,4,1 grid=128 | q=1,1,8 steps=10592512 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    # the GRU forward: (16, 128) has NQ = 1; its workspace and T limit
    ("fwd 256 -1 -1 0 16 128 4 189696 0 0 0 1",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=1,0,0 sizes=132352,231168,189696 | shape not supported by the persistent GRU recurrence (see yt8m_gru_persist_supported)"),
    ("fwd 256 -1 -1 0 32 256 4 559360 0 0 0 1",
     "code=0 ok=1 geo=2,32,1,2,8,1 grid=32 nimg=0 form=fp32 pack=plain SH=0 PD=1 NKB=0 | q=1,1,0 sizes=329984,725248,559360 | "),
    ("fwd 256 -1 -1 0 128 1024 4 7938304 0 0 0 1",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=0 form=fp32 pack=plain SH=0 PD=1 NKB=0 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("fwd 256 -1 -1 0 32 256 4 559359 0 0 0 1",
     "code=-2 ok=1 geo=2,32,1,2,8,1 grid=32 | q=1,1,0 sizes=329984,725248,559360 | workspace too small"),
    ("fwd 256 -1 -1 0 32 256 524288 1152921504606846976 0 0 0 1",
     "code=-2 ok=1 geo=2,32,1,2,8,1 grid=32 | q=1,1,0 sizes=329984,68988111104,51539773696 | T too large"),
    ("fwd 256 -1 -1 0 32 256 524287 1152921504606846976 0 0 0 1",
     "code=0 ok=1 geo=2,32,1,2,8,1 grid=32 nimg=0 form=fp32 pack=plain SH=0 PD=1 NKB=0 | q=1,1,0 sizes=329984,68987979520,51539675392 | "),
    # every knob, one at a time, at (128, 1024), T = 4, per-step workspace, h2 requests (the defaults first)
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 no_persist=1",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 sizes=0,0,0 | shape not supported by the persistent recurrence (see yt8m_lstm_persist_supported)"),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 no_persist=1",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 steps=0 | shape not supported by the persistent backward recurrence (see yt8m_lstm_persist_bwd_supported)"),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 no_persist_bwd=1",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 no_persist_bwd=1",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=0,0,0 steps=10592512 | shape not supported by the persistent backward recurrence (see yt8m_lstm_persist_bwd_supported)"),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 x3=0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 x3=0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 fwd_h2=0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 fwd_h2=0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 bwd_h2=0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 bwd_h2=0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,0,8 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 bwd_rot=0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 bwd_rot=0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 tape_prefetch=0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 tape_prefetch=0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=0 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 cus=128",
     "code=0 ok=1 geo=8,128,1,8,8,2 grid=128 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=2 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 cus=128",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 cus=64",
     "code=0 ok=1 geo=8,128,1,8,8,2 grid=128 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=2 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 cus=64",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 cus_bwd=0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 cus_bwd=0",
     "code=0 ok=1 geo=32,64,4,8,2,1 grid=256 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 cus_bwd=64",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 cus_bwd=64",
     "code=0 ok=1 geo=32,64,1,8,8,1 grid=64 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,4 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 gru=0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,0,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 gru=0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 chain=1",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 chain=1",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 reserved_cus=64",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0 reserved_cus=64",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 7938304 0 0 0 1 gru=0",
     "code=-2 ok=0 geo=0,0,0,0,0,0 grid=0 | q=1,0,1 sizes=4268288,10592512,7938304 | shape not supported by the persistent GRU recurrence (see yt8m_gru_persist_supported)"),
    ("fwd 256 0 -1 0 128 1024 4 10592512 0 0 0 0 cus=128",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 0 0 128 1024 4 10592512 2 0 0 0 cus_bwd=64",
     "code=0 ok=1 geo=32,64,4,8,2,1 grid=256 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 0 1 0 0 bwd_rot=0",
     "code=-2 ok=1 geo=32,64,2,8,4,1 grid=128 | q=1,0,0 steps=10592512 | operand images need the rotated backward epilogue"),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 0 0 1 0 bwd_rot=0",
     "code=-2 ok=1 geo=32,64,2,8,4,1 grid=128 | q=1,0,0 steps=10592512 | row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)"),
    # the three tape-prefetch modes of the calling thread, with the process default on and off
    ("bwd 256 -1 -1 1 128 1024 4 10592512 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 2 128 1024 4 10592512 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=0 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 1 128 1024 4 10592512 2 0 0 0 tape_prefetch=0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 2 128 1024 4 10592512 2 0 0 0 tape_prefetch=0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=0 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 1 128 1024 4 10592512 1 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=bf16 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
]

GPU_TABLE = [
    ("fwd 256 -1 -1 0 16 128 4 231168 0 0 0 0",
     "code=0 ok=1 geo=1,16,1,1,8,0 grid=16 nimg=20 form=fp32 pack=plain SH=1 PD=0 NKB=0 | q=1,0,0 sizes=132352,231168,189696 | "),
    ("fwd 256 -1 -1 0 16 128 4 231168 1 0 0 0",
     "code=0 ok=1 geo=1,16,1,1,8,0 grid=16 nimg=20 form=fp32 pack=plain SH=1 PD=0 NKB=0 | q=1,0,0 sizes=132352,231168,189696 | "),
    ("fwd 256 -1 -1 0 16 128 4 231168 2 0 0 0",
     "code=0 ok=1 geo=1,16,1,1,8,0 grid=16 nimg=20 form=fp32 pack=plain SH=1 PD=0 NKB=0 | q=1,0,0 sizes=132352,231168,189696 | "),
    ("bwd 256 -1 -1 0 16 128 4 231168 0 0 0 0",
     "code=0 ok=1 geo=4,8,1,1,8,0 grid=8 nimg=5 form=fp32 SH=1 PF=0 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=231168 | "),
    ("bwd 256 -1 -1 0 16 128 4 231168 1 0 0 0",
     "code=0 ok=1 geo=4,8,1,1,8,0 grid=8 nimg=5 form=fp32 SH=1 PF=0 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=231168 | "),
    ("bwd 256 -1 -1 0 16 128 4 231168 2 0 0 0",
     "code=0 ok=1 geo=4,8,1,1,8,0 grid=8 nimg=5 form=fp32 SH=1 PF=0 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=231168 | "),
    ("fwd 256 -1 -1 0 16 128 4 132352 0 0 0 0",
     "code=0 ok=1 geo=1,16,1,1,8,0 grid=16 nimg=8 form=fp32 pack=plain SH=1 PD=0 NKB=0 | q=1,0,0 sizes=132352,231168,189696 | "),
    ("fwd 256 -1 -1 0 16 128 4 132352 1 0 0 0",
     "code=0 ok=1 geo=1,16,1,1,8,0 grid=16 nimg=8 form=fp32 pack=plain SH=1 PD=0 NKB=0 | q=1,0,0 sizes=132352,231168,189696 | "),
    ("fwd 256 -1 -1 0 16 128 4 132352 2 0 0 0",
     "code=0 ok=1 geo=1,16,1,1,8,0 grid=16 nimg=8 form=fp32 pack=plain SH=1 PD=0 NKB=0 | q=1,0,0 sizes=132352,231168,189696 | "),
    ("bwd 256 -1 -1 0 16 128 4 132352 0 0 0 0",
     "code=0 ok=1 geo=4,8,1,1,8,0 grid=8 nimg=2 form=fp32 SH=0 PF=0 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=231168 | "),
    ("bwd 256 -1 -1 0 16 128 4 132352 1 0 0 0",
     "code=0 ok=1 geo=4,8,1,1,8,0 grid=8 nimg=2 form=fp32 SH=0 PF=0 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=231168 | "),
    ("bwd 256 -1 -1 0 16 128 4 132352 2 0 0 0",
     "code=0 ok=1 geo=4,8,1,1,8,0 grid=8 nimg=2 form=fp32 SH=0 PF=0 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=231168 | "),
    ("fwd 256 -1 -1 0 64 1024 4 5329152 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,4,8,1 grid=128 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=2167040,5329152,4002048 | "),
    ("fwd 256 -1 -1 0 64 1024 4 5329152 1 0 0 0",
     "code=0 ok=1 geo=8,128,1,4,8,1 grid=128 nimg=20 form=bf16_one_plane pack=x3_one SH=1 PD=1 NKB=4 | q=1,1,1 sizes=2167040,5329152,4002048 | "),
    ("fwd 256 -1 -1 0 64 1024 4 5329152 2 0 0 0",
     "code=0 ok=1 geo=8,128,1,4,8,1 grid=128 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=2167040,5329152,4002048 | "),
    ("bwd 256 -1 -1 0 64 1024 4 5329152 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    ("bwd 256 -1 -1 0 64 1024 4 5329152 1 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    ("bwd 256 -1 -1 0 64 1024 4 5329152 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    ("fwd 256 -1 -1 0 64 1024 4 2167040 0 0 0 0",
     "code=0 ok=1 geo=8,128,1,4,8,1 grid=128 nimg=8 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=2167040,5329152,4002048 | "),
    ("fwd 256 -1 -1 0 64 1024 4 2167040 1 0 0 0",
     "code=0 ok=1 geo=8,128,1,4,8,1 grid=128 nimg=8 form=bf16_one_plane pack=x3_one SH=1 PD=1 NKB=4 | q=1,1,1 sizes=2167040,5329152,4002048 | "),
    ("fwd 256 -1 -1 0 64 1024 4 2167040 2 0 0 0",
     "code=0 ok=1 geo=8,128,1,4,8,1 grid=128 nimg=8 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=2167040,5329152,4002048 | "),
    ("bwd 256 -1 -1 0 64 1024 4 2167040 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=2 form=fp32 SH=0 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    ("bwd 256 -1 -1 0 64 1024 4 2167040 1 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=2 form=fp32 SH=0 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    ("bwd 256 -1 -1 0 64 1024 4 2167040 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=2 form=fp32 SH=0 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    ("fwd 256 -1 -1 0 128 512 4 5333248 0 0 0 0",
     "code=0 ok=1 geo=4,64,2,8,4,1 grid=128 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=2 | q=1,1,1 sizes=2171136,5333248,4006144 | "),
    ("fwd 256 -1 -1 0 128 512 4 5333248 1 0 0 0",
     "code=0 ok=1 geo=4,64,2,8,4,1 grid=128 nimg=20 form=bf16_one_plane pack=x3_one SH=1 PD=1 NKB=2 | q=1,1,1 sizes=2171136,5333248,4006144 | "),
    ("fwd 256 -1 -1 0 128 512 4 5333248 2 0 0 0",
     "code=0 ok=1 geo=4,64,2,8,4,1 grid=128 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=2 | q=1,1,1 sizes=2171136,5333248,4006144 | "),
    ("bwd 256 -1 -1 0 128 512 4 5333248 0 0 0 0",
     "code=0 ok=1 geo=16,32,4,8,2,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5333248 | "),
    ("bwd 256 -1 -1 0 128 512 4 5333248 1 0 0 0",
     "code=0 ok=1 geo=16,32,4,8,2,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5333248 | "),
    ("bwd 256 -1 -1 0 128 512 4 5333248 2 0 0 0",
     "code=0 ok=1 geo=16,32,4,8,2,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5333248 | "),
    ("fwd 256 -1 -1 0 128 512 4 2171136 0 0 0 0",
     "code=0 ok=1 geo=4,64,2,8,4,1 grid=128 nimg=8 form=x3_six pack=x3_three SH=1 PD=1 NKB=2 | q=1,1,1 sizes=2171136,5333248,4006144 | "),
    ("fwd 256 -1 -1 0 128 512 4 2171136 1 0 0 0",
     "code=0 ok=1 geo=4,64,2,8,4,1 grid=128 nimg=8 form=bf16_one_plane pack=x3_one SH=1 PD=1 NKB=2 | q=1,1,1 sizes=2171136,5333248,4006144 | "),
    ("fwd 256 -1 -1 0 128 512 4 2171136 2 0 0 0",
     "code=0 ok=1 geo=4,64,2,8,4,1 grid=128 nimg=8 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=2 | q=1,1,1 sizes=2171136,5333248,4006144 | "),
    ("bwd 256 -1 -1 0 128 512 4 2171136 0 0 0 0",
     "code=0 ok=1 geo=16,32,4,8,2,1 grid=128 nimg=2 form=fp32 SH=0 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5333248 | "),
    ("bwd 256 -1 -1 0 128 512 4 2171136 1 0 0 0",
     "code=0 ok=1 geo=16,32,4,8,2,1 grid=128 nimg=2 form=fp32 SH=0 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5333248 | "),
    ("bwd 256 -1 -1 0 128 512 4 2171136 2 0 0 0",
     "code=0 ok=1 geo=16,32,4,8,2,1 grid=128 nimg=2 form=fp32 SH=0 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5333248 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 1 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=bf16_one_plane pack=x3_one SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("fwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=20 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 1 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=bf16 SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("fwd 256 -1 -1 0 128 1024 4 4268288 0 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=8 form=x3_six pack=x3_three SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("fwd 256 -1 -1 0 128 1024 4 4268288 1 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=8 form=bf16_one_plane pack=x3_one SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("fwd 256 -1 -1 0 128 1024 4 4268288 2 0 0 0",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=8 form=h2_two_plane pack=x3_two_f16 SH=1 PD=1 NKB=4 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
    ("bwd 256 -1 -1 0 128 1024 4 4268288 0 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=2 form=fp32 SH=0 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 4268288 1 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=2 form=fp32 SH=0 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 4268288 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=2 form=fp32 SH=0 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("fwd 256 -1 -1 0 48 768 4 3027200 0 0 0 0",
     "code=0 ok=1 geo=6,96,1,3,8,1 grid=96 nimg=20 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=1248512,3027200,2280704 | "),
    ("fwd 256 -1 -1 0 48 768 4 3027200 1 0 0 0",
     "code=0 ok=1 geo=6,96,1,3,8,1 grid=96 nimg=20 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=1248512,3027200,2280704 | "),
    ("fwd 256 -1 -1 0 48 768 4 3027200 2 0 0 0",
     "code=0 ok=1 geo=6,96,1,3,8,1 grid=96 nimg=20 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=1248512,3027200,2280704 | "),
    ("bwd 256 -1 -1 0 48 768 4 3027200 0 0 0 0",
     "code=0 ok=1 geo=24,48,1,3,8,1 grid=48 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=3027200 | "),
    ("bwd 256 -1 -1 0 48 768 4 3027200 1 0 0 0",
     "code=0 ok=1 geo=24,48,1,3,8,1 grid=48 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=3027200 | "),
    ("bwd 256 -1 -1 0 48 768 4 3027200 2 0 0 0",
     "code=0 ok=1 geo=24,48,1,3,8,1 grid=48 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=3027200 | "),
    ("fwd 256 -1 -1 0 48 768 4 1248512 0 0 0 0",
     "code=0 ok=1 geo=6,96,1,3,8,1 grid=96 nimg=8 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=1248512,3027200,2280704 | "),
    ("fwd 256 -1 -1 0 48 768 4 1248512 1 0 0 0",
     "code=0 ok=1 geo=6,96,1,3,8,1 grid=96 nimg=8 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=1248512,3027200,2280704 | "),
    ("fwd 256 -1 -1 0 48 768 4 1248512 2 0 0 0",
     "code=0 ok=1 geo=6,96,1,3,8,1 grid=96 nimg=8 form=fp32 pack=plain SH=1 PD=1 NKB=0 | q=1,1,0 sizes=1248512,3027200,2280704 | "),
    ("bwd 256 -1 -1 0 48 768 4 1248512 0 0 0 0",
     "code=0 ok=1 geo=24,48,1,3,8,1 grid=48 nimg=2 form=fp32 SH=0 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=3027200 | "),
    ("bwd 256 -1 -1 0 48 768 4 1248512 1 0 0 0",
     "code=0 ok=1 geo=24,48,1,3,8,1 grid=48 nimg=2 form=fp32 SH=0 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=3027200 | "),
    ("bwd 256 -1 -1 0 48 768 4 1248512 2 0 0 0",
     "code=0 ok=1 geo=24,48,1,3,8,1 grid=48 nimg=2 form=fp32 SH=0 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=3027200 | "),
    ("bwd 256 -1 -1 0 128 1024 4 10592512 0 1 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=images SH=1 PF=1 ROT=1 TPF=0 sc=0,0 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 0 128 1024 4 4268288 0 1 0 0",
     "code=-2 ok=1 geo=32,64,2,8,4,1 grid=128 | q=1,1,8 steps=10592512 | operand images need one exchange image per step"),
    ("bwd 256 -1 -1 0 64 1024 4 5329152 0 1 0 0",
     "code=-2 ok=1 geo=32,64,2,4,4,1 grid=128 | q=1,0,0 steps=5329152 | operand images need the rotated backward epilogue"),
    ("bwd 256 -1 -1 1 128 1024 4 10592512 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=1 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 1 64 1024 4 5329152 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    ("bwd 256 -1 -1 2 128 1024 4 10592512 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,8,4,1 grid=128 nimg=5 form=h2 SH=1 PF=1 ROT=1 TPF=0 sc=10494208,32768 | q=1,1,8 steps=10592512 | "),
    ("bwd 256 -1 -1 2 64 1024 4 5329152 2 0 0 0",
     "code=0 ok=1 geo=32,64,2,4,4,1 grid=128 nimg=5 form=fp32 SH=1 PF=1 ROT=0 TPF=0 sc=0,0 | q=1,0,0 steps=5329152 | "),
    ("fwd 256 -1 -1 0 32 256 4 559360 0 0 0 1",
     "code=0 ok=1 geo=2,32,1,2,8,1 grid=32 nimg=0 form=fp32 pack=plain SH=0 PD=1 NKB=0 | q=1,1,0 sizes=329984,725248,559360 | "),
    ("fwd 256 -1 -1 0 128 1024 4 7938304 0 0 0 1",
     "code=0 ok=1 geo=8,128,2,8,4,1 grid=256 nimg=0 form=fp32 pack=plain SH=0 PD=1 NKB=0 | q=1,1,1 sizes=4268288,10592512,7938304 | "),
]

# YT8M_* variable -> (field, value when unset, {text: value})
KNOB_ENV = {
    "YT8M_NO_PERSIST": ("no_persist", 0, {"0": 1, "1": 1}),                  # set, whatever the value
    "YT8M_NO_PERSIST_BWD": ("no_persist_bwd", 0, {"0": 1, "1": 1}),
    "YT8M_PERSIST_X3": ("x3", 1, {"0": 0, "1": 1}),
    "YT8M_PERSIST_FWD_H2": ("fwd_h2", 1, {"0": 0, "1": 1}),
    "YT8M_PERSIST_BWD_H2": ("bwd_h2", 1, {"0": 0, "1": 1}),
    "YT8M_BWD_ROT": ("bwd_rot", 1, {"0": 0, "1": 1}),
    "YT8M_PERSIST_TAPE_PREFETCH": ("tape_prefetch", 1, {"0": 0, "1": 1}),
    "YT8M_PERSIST_CUS": ("cus", 0, {"0": 0, "128": 128}),
    "YT8M_PERSIST_CUS_BWD": ("cus_bwd", 128, {"0": 0, "64": 64}),
    "YT8M_GRU_PERSIST": ("gru", 1, {"0": 0, "1": 1}),
    "YT8M_PERSIST_CHAIN": ("chain", 0, {"0": 1, "1": 1}),
    "YT8M_PERSIST_RESERVED_CUS": ("reserved_cus", 0, {"0": 0, "64": 64}),
}


def fields(expected):
    """'code=0 ok=1 geo=... | q=... | message' -> dict of strings (+ 'why')."""
    plan, q, why = expected.split(" | ")
    d = dict(kv.split("=") for kv in (plan + " " + q).split())
    d["why"] = why
    return d


def instantiations(case, expected):
    """The kernels the launch of a table row runs, as a kernel trace names them (every template argument spelled out)."""
    f = fields(expected)
    if f["code"] != "0":
        return []
    t = case.split()
    NQ = f["geo"].split(",")[0]
    b = lambda v: "true" if v == "1" else "false"
    if t[0] == "fwd":
        if t[12] == "1":
            return ["hx_pack_kernel", "gru_persist_fwd_kernel<%s, %s>" % (NQ, f["PD"])]
        pack = {"plain": "hx_pack_kernel", "x3_three": "hx_pack_x3_kernel<3, false>", "x3_one": "hx_pack_x3_kernel<1, false>",
                "x3_two_f16": "hx_pack_x3_kernel<2, true>"}[f["pack"]]
        main = {"fp32": "lstm_persist_fwd_kernel<%s, %s, %s>" % (NQ, f["PD"], b(f["SH"])),
                "x3_six": "lstm_persist_fwd_x3_kernel<%s, 3, false>" % f["NKB"],
                "bf16_one_plane": "lstm_persist_fwd_x3_kernel<%s, 1, false>" % f["NKB"],
                "h2_two_plane": "lstm_persist_fwd_x3_kernel<%s, 2, true>" % f["NKB"]}[f["form"]]
        return [pack, main]
    form = f["form"]
    # <NQB, PF, SH, ROT, IMG, BF, H2, TPF>
    return ["lstm_persist_bwd_kernel<%s, %s, %s, %s, %s, %s, %s, %s>" % (NQ, b(f["PF"]), b(f["SH"]), b(f["ROT"]), b(str(int(form == "images"))),
                                                                      b(str(int(form == "bf16"))), b(str(int(form == "h2"))), b(f["TPF"]))]


def _host_cxx():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cc)
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    cxx = _host_cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler in this environment")
    exe = str(tmp_path_factory.mktemp("persist_plan") / "persist_plan_main")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "youtube-8m_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "persist_plan_main.cpp")], check=True, capture_output=True, text=True)
    return exe


def _run(exe, cases, env=None):
    out = subprocess.run([exe], input="\n".join(cases) + "\n", check=True, capture_output=True, text=True, env=env).stdout.splitlines()
    assert len(out) == len(cases)
    return [ln.rstrip() for ln in out]


def test_the_header_needs_no_hip():
    text = open(os.path.join(ROOT, "youtube-8m_amd", "csrc", "persist_plan.h")).read()
    assert "hip_runtime" not in text and "common.h" not in text
    assert text.count("getenv") == 3 + 1            # the three readers inside persist_knobs_from_env, and the sentence that says so


def test_plans_equal_the_table(plan_program):
    assert len(dict(TABLE)) == len(TABLE) and len(dict(GPU_TABLE)) == len(GPU_TABLE)
    assert all(dict(TABLE).get(c, e) == e for c, e in GPU_TABLE)           # rows the two lists share
    rows = TABLE + GPU_TABLE
    got = _run(plan_program, [c for c, _ in rows])
    wrong = [(c, want, g) for (c, want), g in zip(rows, got) if g != want.rstrip()]
    assert not wrong, "\n".join("%s\n  want %s\n  got  %s" % w for w in wrong[:10])


def test_queries_agree_with_the_launch_they_describe():
    """For every row on a per-step workspace (sizes[1]): the forward query is 1 exactly where a plain request gets the six-product form,
    the backward query exactly where an h2 request gets the f16 form; supported exactly where the shape is not refused; the images rows
    are positive exactly where an images request on that workspace is granted."""
    seen = set()
    for case, expected in TABLE + GPU_TABLE:
        t, f = case.split(), fields(expected)
        if t[0] == "fwd":
            if t[12] == "1":
                if f["why"].startswith("shape not supported") or f["code"] == "0":
                    assert (f["code"] == "0") == (f["q"].split(",")[1] == "1"), case
                continue
            assert (f["ok"] == "1") == (f["q"].split(",")[0] == "1"), case
            steps = f["sizes"].split(",")[1]
            if f["code"] == "0" and t[8] == steps and t[9] == "0":
                assert (f["form"] == "x3_six") == (f["q"].split(",")[2] == "1"), case
                seen.add(("fwd", f["form"] == "x3_six"))
        else:
            q = f["q"].split(",")
            assert (f["ok"] == "1") == (q[0] == "1"), case
            if f["ok"] == "1" and t[8] == f["steps"] and t[11] == "0":
                if t[9] == "2" and t[10] == "0":
                    assert (f["form"] == "h2") == (q[1] == "1"), case
                    seen.add(("bwd", f["form"] == "h2"))
                if t[10] == "1" and int(t[5]) % 16 == 0:
                    assert (f["code"] == "0" and f["form"] == "images") == (int(q[2]) > 0), case
                    seen.add(("img", f["code"] == "0"))
    assert seen == {(d, v) for d in ("fwd", "bwd", "img") for v in (False, True)}


@pytest.mark.parametrize("var", sorted(KNOB_ENV))
def test_each_knob_is_read_from_its_variable(plan_program, var):
    field, unset, values = KNOB_ENV[var]
    base = {k: v for k, v in os.environ.items() if not k.startswith("YT8M_")}
    defaults = dict(kv.split("=") for kv in _run(plan_program, ["env"], env=base)[0].split())
    assert defaults == {"no_persist": "0", "no_persist_bwd": "0", "x3": "1", "fwd_h2": "1", "bwd_h2": "1", "bwd_rot": "1", "tape_prefetch": "1",
                        "cus": "0", "cus_bwd": "128", "gru": "1", "chain": "0", "reserved_cus": "0"}
    assert defaults[field] == str(unset)
    for text, value in values.items():
        got = dict(kv.split("=") for kv in _run(plan_program, ["env"], env=dict(base, **{var: text}))[0].split())
        assert got == dict(defaults, **{field: str(value)}), (var, text)


def test_recorded_instantiations_are_the_ones_the_table_names():
    """tests/golden/persist_forms_seen.txt -- what a kernel trace of tests/test_gpu_persist_forms.py showed on a 256-CU MI355X -- holds
    every instantiation the GPU rows name and no other persistent kernel."""
    named = {k for case, expected in GPU_TABLE for k in instantiations(case, expected)}
    seen = {ln.strip() for ln in open(os.path.join(ROOT, "tests", "golden", "persist_forms_seen.txt")) if ln.strip()}
    assert seen == named, (sorted(named - seen), sorted(seen - named))
