"""Diagnostic: a gated connection alone, timed with HIP events -- CextNet's conv_t_1 (8 x 8 x 128 -> 128,
T = 20) or, with `dense`, its dense1 (C = 128, H W = 16 -> 512, T = 20: 20 480 rows at B = 1024):
  [SNNQP_DIAG_LIB=...] python tools/gated_time.py [dense] [B] [bits]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from snnquantprune_amd import _lib as L, ops, packing, synthetic as syn
from snnquantprune_amd.quant import QuantDesc
dev = torch.device("cuda:0")
argv = sys.argv[1:]
dense = argv[:1] == ["dense"]
argv = argv[1:] if dense else argv
B = int(argv[0]) if len(argv) > 0 else 1024
bits = int(argv[1]) if len(argv) > 1 else 4
T, C = 20, 128
H, W, N = (4, 4, 512) if dense else (8, 8, 128)
leaf = syn.quant_leaf((C * H * W, N) if dense else (3, 3, C, N), 5.0, 971, True, 0.9 if bits == 4 else 0.3)
a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
pk = packing.PackedKernel(torch.from_numpy(leaf["kernel"]).to(dev), QuantDesc(L.Q_DUQ, bits, a, c, float(2 ** (bits - 1) - 1), float(np.float32(c)), True),
                          torch.from_numpy(leaf["prune_0"]["mask"]).to(dev))
w = pk.int_weight()
s = ops.pack_bits((torch.rand((T, B, H, W, C), device=dev) < 0.2).to(torch.uint8))
gate = torch.sigmoid(torch.randn((T, B, C), device=dev))
if dense:
  x, packed = ops.GatedSpikes(s, gate, flat=True), pk.gated_dense_codes(C, H * W)
  run = lambda: ops.dense_gated_forward(x, w, packed)
else:
  x, packed = ops.GatedSpikes(s, gate), pk.gated_codes()
  geom = ops.ConvGeom(H, W, C, N, 3, 3, pad=((1, 1), (1, 1)))
  run = lambda: ops.conv_gated_forward(x, geom, w, packed)
for _ in range(3):
  y = run()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
n = 100 if dense else 10               # (the dense launch is a tenth of the conv one)
e0.record()
for _ in range(n):
  y = run()
e1.record()
torch.cuda.synchronize()
print("%s %s_gated %dx%dx%d->%d B=%d T=%d %d-bit: %.4f ms per launch (checksum %.6g)" % (
    os.environ.get("SNNQP_DIAG_LIB", "product"), "dense" if dense else "conv", H, W, C, N, B, T, bits,
    e0.elapsed_time(e1) / n, float(y.double().sum())))
