"""Builder tool (GPU box, under rocprofv3 --pmc): a few launches of one fused-ResBlock-step kernel per shape on random data (sbv2_debug_respair).
  python3 tools/respair_pmc.py [variant]      variant 0 = respair_cl, 1 = the default dispatch's kernel, 2 = respair_clx"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sbv2_api_amd import _lib
l = _lib.lib()
variant = int(sys.argv[1]) if len(sys.argv) > 1 else 1
P = lambda a: a.ctypes.data_as(_lib.f32p)
for (c, k, d, L) in ((32, 7, 3, 229632 * 16), (16, 7, 3, 459264 * 16), (64, 7, 3, 114816 * 16)):
    rng = np.random.default_rng(c + k)
    x = rng.standard_normal((L, c), dtype=np.float32)
    w1, w2 = ((rng.standard_normal((c, c, k)) / np.sqrt(k * c)).astype(np.float32) for _ in range(2))
    b1, b2 = (rng.standard_normal(c).astype(np.float32) for _ in range(2))
    y = np.zeros((L, c), np.float32)
    for _ in range(3):
        _lib.check(l.sbv2_debug_respair(0, P(x), P(w1), P(w2), P(b1), P(b2), c, L, k, d, None, 1, 1.0, 0, variant, P(y)))
    print(c, k, d, flush=True)
