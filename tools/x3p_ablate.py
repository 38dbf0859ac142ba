"""The hidden weight grad alone (2048 x 2048 x 6400, split2h, both operands k-major, fp32 store) on gemm_x3p:
the critic's launch (E = 2) and the actor's (E = 1, split-K by the launcher's choice + its reduce launch), with
the pipelined main loop and the unpipelined one (bit 16), each as is and with the ablation bits 1 (no refill
DMA), 2 (no MFMAs), 8 (refill issued up front).  Ablated results are wrong; only the time matters.
usage: python tools/x3p_ablate.py [iters]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtrl_amd import _lib as L

lib = L.load()
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
M, N, K = 2048, 2048, 6400
H2, KMAJOR, AUTO_SPLITS = 1 << 13, 3 << 8, 255 << 16
for rep in range(2):
    for E in (2, 1):
        for loop, bit in (("pipelined", 0), ("unpipelined", 16)):
            for abl in (0, 1, 2, 8):
                lib.mtsac_debug_x3p_geo(255 | ((bit | abl) << 8))
                ms = ctypes.c_double()
                L.check(lib.mtsac_debug_gemm_x3p_bench(0 | KMAJOR | H2 | (AUTO_SPLITS if E == 1 else 0), E, M, N, K, iters,
                                                       ctypes.byref(ms)))
                lib.mtsac_debug_x3p_geo(-1)
                tf = 2.0 * M * N * K * E / (ms.value * 1e-3) / 1e12
                print(f"E {E} {loop:11s} abl {abl}: {ms.value * 1e3:7.1f} us {tf:6.1f} TF ({tf / 833.33:.3f})", flush=True)
