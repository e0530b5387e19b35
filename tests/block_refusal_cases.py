"""What the host side of the fused blocks refuses, call by call: the table of
tests/test_block_refusals_cpu.py.  No GPU and no device memory: every pointer is made up, and every
row is stopped by a host check before any launch (an empty batch, which returns SNNQP_OK, is the one
exception).  A row that passed every check would launch a kernel on these pointers on a machine that
has a GPU, so there is none.

A row names an entry point, what it changes in that entry point's base call (BASE: a call that would
launch), the return code and the whole text of snnqp_last_error() -- None where the code is
SNNQP_OK, which leaves the text as it was.  `fallback`, where given, is the reason
snnqp_fallback_counts() holds after the call ("" for none: the counters are reset before every row).

The rows cover every refusal a public entry point can reach in the dispatch (csrc/blocks.hip), the
five *_unsupported predicates, the entry checks and the direct-form kernel's own checks, and the order
of the checks where two rules are broken at once.  Routes that end in a launch are told apart by the
refusal of the kernel's own run function ("dense wide: null pointer" against "dense mfma: null
pointer"): the row drops s_out."""
from collections import namedtuple

from snnquantprune_amd import _lib as L

OK, EINVAL, EUNSUP = L.OK, L.EINVAL, L.EUNSUPPORTED
P = 0x10000          # a made-up device pointer, 16-byte aligned; host code never reads through it

GEOM = dict(H=8, W=8, Cin=32, Cout=32, KH=3, KW=3, stride_h=1, stride_w=1, pad_h_lo=1, pad_h_hi=1,
            pad_w_lo=1, pad_w_hi=1, in_dil_h=1, in_dil_w=1, k_dil_h=1, k_dil_w=1, groups=1)
GEOM3 = dict(D=4, H=8, W=8, Cin=32, Cout=32, KD=3, KH=3, KW=3, stride=(1, 1, 1), pad_lo=(1, 1, 1),
             pad_hi=(1, 1, 1), in_dil=(1, 1, 1), k_dil=(1, 1, 1), groups=1)
WEIGHT = dict(wtype=L.W_I8, w=P, L=7.0, m=0.5, abs_sum_max=100, code_max=127, col_sum=None, wt_fp6=None,
              min_current_bits=0, ch_stack_max=0, ch_slots=None, wt_cin=0, cout_fire=0)
NRN = dict(kind=L.NEURON_MULTI_STEP_LIF, k=2.0, v_threshold=1.0, v_reset=0.0, decay=None)
BN = dict(mean=P, mul=P, bias=P, flags=0)
STRUCTS = {"g": (L.ConvGeomT, GEOM), "g3": (L.Conv3dGeomT, GEOM3), "w": (L.WeightT, WEIGHT),
           "w1": (L.WeightT, WEIGHT), "w2": (L.WeightT, WEIGHT), "bn": (L.BnT, BN), "nrn": (L.NeuronT, NRN),
           "nrn1": (L.NeuronT, NRN), "nrn2": (L.NeuronT, NRN)}

_BLOCK = dict(x=P, in_type=L.BITS, xs_t=64, xs_b=256, T=4, B=2)
_TAIL = dict(bn=None, nrn={}, u0=None, u_out=None, s_out=P, s_type=L.BITS)
_DENSE = dict(x=P, in_type=L.BITS, xs_t=2, xs_b=8, T=4, B=2, K=64, N=64, w={}, wt=P, **_TAIL)
_CONV_FWD = dict(x=P, in_type=L.BITS, NB=2, g={}, w={})

# entry -> (symbol, the arguments in order with the values of a call that would launch; {} stands
# for the default structure of that name, None for a null pointer)
BASE = {
    "conv_lif": ("snnqp_conv_lif_forward", dict(
        _BLOCK, g={}, w={}, wt=P, **_TAIL, pool=1, impl=L.IMPL_AUTO, x_max=1, x_seen=None, x_flags=None,
        stream=None)),
    "conv_pred": ("snnqp_conv_lif_forward_pred", dict(
        pred=P, x=P, in_type=L.U8, xs_t=128, xs_b=512, T=4, B=2, g=dict(Cin=2), w={}, wt=None, **_TAIL,
        pool=1, x_max=1, x_seen=None, x_flags=None, stream=None)),
    "conv_if": ("snnqp_conv_lif_forward_if", dict(
        pred=P, **_BLOCK, g={}, w={}, **_TAIL, pool=1, stream=None)),
    "dense_if": ("snnqp_dense_lif_forward_if", dict(
        pred=P, x=P, in_type=L.BITS, xs_t=2, xs_b=8, T=4, B=2, K=64, N=64, w={}, **_TAIL, stream=None)),
    "dense": ("snnqp_dense_lif_forward", dict(_DENSE, impl=L.IMPL_AUTO, stream=None)),
    "dense_ws": ("snnqp_dense_lif_forward_ws", dict(
        _DENSE, impl=L.IMPL_AUTO, x_flags=None, ws=None, ws_bytes=0, stream=None)),
    "head": ("snnqp_dense_head_forward", dict(
        x=P, in_type=L.BITS, xs_t=2, xs_b=8, T=4, B=2, K=64, N1=256, w1={}, wt1=P, nrn1={}, N2=20, w2={},
        wt2=P, nrn2={}, group=2, s1_out=None, s2_out=None, logits=P, x_flags=None, ws=None, ws_bytes=0,
        stream=None)),
    "conv_fwd": ("snnqp_conv_forward", dict(_CONV_FWD, y=P, acc=None, stream=None)),
    "conv_ex": ("snnqp_conv_forward_ex", dict(
        _CONV_FWD, wt=P, y=P, acc=None, impl=L.IMPL_AUTO, stream=None)),
    "conv_fwd_if": ("snnqp_conv_forward_if", dict(pred=P, **_CONV_FWD, y=P, stream=None)),
    "conv3d": ("snnqp_conv3d_lif_forward", dict(
        pred=None, x=P, in_type=L.BITS, xs_t=256, xs_b=1024, T=4, B=2, g3={}, w={}, **_TAIL, stream=None)),
    "half_group": ("snnqp_conv_event_half_group", dict(
        in_type=L.EV1, T=4, g=dict(Cin=2), w={}, nrn={}, has_state=0, pool=1, x_max=1)),
    "dequant_form": ("snnqp_conv_dequant_form", dict(w={}, nrn={})),
}

Row = namedtuple("Row", "name entry change code text fallback")
ROWS = []


def row(name, entry, code, text, fallback=None, **change):
  assert (text is None) == (code == OK), name
  ROWS.append(Row(name, entry, change, code, text, fallback))


def _struct(kind, fields):
  cls, base = STRUCTS[kind]
  v = dict(base, **fields)
  if cls is L.Conv3dGeomT:
    v = {k: (L.c_int32 * 3)(*x) if isinstance(x, tuple) else x for k, x in v.items()}
  return cls(*[v[n] for n, _ in cls._fields_])


def call_args(r):
  """(symbol, ctypes arguments, the structures they point to -- to be kept alive over the call)."""
  import ctypes
  symbol, base = BASE[r.entry]
  assert set(r.change) <= set(base), (r.name, set(r.change) - set(base))
  args, keep = [], []
  for name, v in base.items():
    if name in STRUCTS:
      c = r.change.get(name, {})
      v = None if c is None or (v is None and name not in r.change) else _struct(name, dict(v or {}, **c))
      keep.append(v)
      args.append(None if v is None else ctypes.byref(v))
    else:
      args.append(r.change.get(name, v))
  return symbol, args, keep


U8W = dict(col_sum=P)                       # weights a uint8 / float32 dense input needs
FP6W = dict(wt_fp6=P, code_max=7)           # weights the fp6 dense kernel takes
LIF0 = dict(kind=L.NEURON_LIF)              # LIF without its decay vector
BADBN = dict(flags=0x7F3)
BN_NULL = "batch-norm descriptor with null arrays"
BN_FLAGS = "batch-norm descriptor with unknown flag bits 0x7f3 (built against another snnqp.h?)"
L_MSG = "dequant L must be >= 1"
G_NULL = "generic block: null pointer"
INT_IN = ("int8 codes need integer-typed input (U8/BITS); pass the fake-quantised float kernel for "
          "float32 input")

# ---- snnqp_conv_lif_forward: the entry checks ---------------------------------------------------------
CL = "conv_lif_forward: "
row("cl_null_g", "conv_lif", EINVAL, CL + "null descriptor", g=None)
row("cl_null_w", "conv_lif", EINVAL, CL + "null descriptor", w=None)
row("cl_null_nrn", "conv_lif", EINVAL, CL + "null descriptor", nrn=None)
F32_FLAGS = CL + "float32 input into integer codes needs x_flags (snnqp.h)"
row("cl_f32_no_flags", "conv_lif", EINVAL, F32_FLAGS, in_type=L.F32, g=dict(Cin=2))
row("cl_f32_no_flags_then_kind", "conv_lif", EINVAL, F32_FLAGS, in_type=L.F32, nrn=dict(kind=9))
row("cl_kind_9", "conv_lif", EINVAL, CL + "unknown neuron kind 9", nrn=dict(kind=9))
row("cl_kind_none", "conv_lif", EINVAL, CL + "unknown neuron kind 0", nrn=dict(kind=0))
row("cl_kind_then_pool", "conv_lif", EINVAL, CL + "unknown neuron kind 4", nrn=dict(kind=4), pool=3)
row("cl_pool_3", "conv_lif", EINVAL, CL + "pool must be 1 or 2", pool=3)
row("cl_pool_0", "conv_lif", EINVAL, CL + "pool must be 1 or 2", pool=0)
row("cl_pool_then_impl", "conv_lif", EINVAL, CL + "pool must be 1 or 2", pool=3, impl=7)
row("cl_impl_3", "conv_lif", EINVAL, CL + "unknown impl 3", impl=3)
row("cl_impl_neg", "conv_lif", EINVAL, CL + "unknown impl -1", impl=-1)
row("cl_impl_then_geometry", "conv_lif", EINVAL, CL + "unknown impl 3", impl=3, g=dict(KH=5))

# ---- conv3x3_mfma_unsupported, every branch (impl = MFMA reports the reason) ----------------------------
CM = CL + "MFMA kernel: "
BIG_U8 = dict(Cin=2, H=32768, W=32768)
for name, why, change in [
    ("f32_weights", "weights are not int8 codes", dict(w=dict(wtype=L.W_F32))),
    ("kh5", "kernel is not 3x3", dict(g=dict(KH=5, pad_h_lo=2, pad_h_hi=2))),
    ("kw1", "kernel is not 3x3", dict(g=dict(KW=1))),
    ("stride_h", "stride is not 1", dict(g=dict(stride_h=2))),
    ("stride_w", "stride is not 1", dict(g=dict(stride_w=2))),
    ("pad_h_lo", "padding is not ((1,1),(1,1))", dict(g=dict(pad_h_lo=0))),
    ("pad_h_hi", "padding is not ((1,1),(1,1))", dict(g=dict(pad_h_hi=2))),
    ("pad_w_lo", "padding is not ((1,1),(1,1))", dict(g=dict(pad_w_lo=2))),
    ("pad_w_hi", "padding is not ((1,1),(1,1))", dict(g=dict(pad_w_hi=0))),
    ("in_dil_h", "dilated convolution", dict(g=dict(in_dil_h=2))),
    ("in_dil_w", "dilated convolution", dict(g=dict(in_dil_w=2))),
    ("k_dil_h", "dilated convolution", dict(g=dict(k_dil_h=2))),
    ("k_dil_w", "dilated convolution", dict(g=dict(k_dil_w=2))),
    ("groups", "grouped convolution", dict(g=dict(groups=2))),
    ("h0", "empty image", dict(g=dict(H=0))),
    ("w_neg", "empty image", dict(g=dict(W=-1))),
    ("cout0", "no output channels", dict(g=dict(Cout=0))),
    ("s_f32", "spike output must be bit-packed", dict(s_type=L.F32)),
    ("bits_cin0", "bit input needs Cin <= 128", dict(g=dict(Cin=0))),
    ("bits_cin129", "bit input needs Cin <= 128", dict(g=dict(Cin=129))),
    ("u8_cin32", "u8 input needs Cin == 2", dict(in_type=L.U8)),
    ("u8_2gib", "u8 frame of 2 GiB or more", dict(in_type=L.U8, g=BIG_U8)),
    ("ev1_cin3", "EV1 frames have Cin == 2", dict(in_type=L.EV1, g=dict(Cin=3))),
    ("ev1_2gib", "EV1 frame of 2^31 bits or more", dict(in_type=L.EV1, g=BIG_U8)),
    ("ev4_cin1", "EV4 frames have Cin == 2", dict(in_type=L.EV4, g=dict(Cin=1))),
    ("ev4_2gib", "EV4 frame of 2 GiB or more", dict(in_type=L.EV4, g=dict(Cin=2, H=65536, W=32768))),
    ("f32_cin32", "float32 input into integer codes needs Cin == 2", dict(in_type=L.F32, x_flags=P)),
    ("f32_2gib", "float32 frame of 2 GiB or more",
     dict(in_type=L.F32, x_flags=P, g=dict(Cin=2, H=16384, W=16384))),
    ("in_type_7", "input must be BITS, U8, EV1, EV4 or (Cin == 2) F32", dict(in_type=7)),
    ("lif_no_decay", "LIF without decay", dict(nrn=LIF0)),
    ("no_wt", "MFMA-tiled codes `wt` not given", dict(wt=None)),
    # two at once: the first in the predicate's order is the one reported
    ("f32_weights_then_kh5", "weights are not int8 codes", dict(w=dict(wtype=L.W_F32), g=dict(KH=5))),
    ("kh5_then_stride", "kernel is not 3x3", dict(g=dict(KH=5, stride_h=2))),
    ("groups_then_h0", "grouped convolution", dict(g=dict(groups=2, H=0))),
    ("cout0_then_s_f32", "no output channels", dict(g=dict(Cout=0), s_type=L.F32)),
    ("s_f32_then_cin129", "spike output must be bit-packed", dict(s_type=L.F32, g=dict(Cin=129))),
    ("cin129_then_lif", "bit input needs Cin <= 128", dict(g=dict(Cin=129), nrn=LIF0)),
    ("lif_then_no_wt", "LIF without decay", dict(nrn=LIF0, wt=None)),
]:
  row("cm_" + name, "conv_lif", EUNSUP, CM + why, impl=L.IMPL_MFMA, **change)

# ---- run_conv3x3_mfma behind snnqp_conv_lif_forward --------------------------------------------------
C3 = "conv3x3 mfma: "
WT_CIN = C3 + "wt_cin must be a multiple of 32 in [Cin, 128]"
row("c3_null_codes", "conv_lif", EINVAL, C3 + "null pointer", w=dict(w=None))
row("c3_null_x", "conv_lif", EINVAL, C3 + "null pointer", x=None)
row("c3_null_s_out", "conv_lif", EINVAL, C3 + "null pointer", s_out=None, impl=L.IMPL_MFMA)
row("c3_null_then_negative", "conv_lif", EINVAL, C3 + "null pointer", x=None, T=-1)
row("c3_null_then_wt_cin", "conv_lif", EINVAL, C3 + "null pointer", s_out=None, w=dict(wt_cin=40))
row("c3_null_codes_empty", "conv_lif", EINVAL, C3 + "null pointer", w=dict(w=None), T=0)
row("c3_empty_t", "conv_lif", OK, None, x=None, s_out=None, T=0)
row("c3_empty_b", "conv_lif", OK, None, x=None, B=0)
row("c3_wt_cin_40", "conv_lif", EINVAL, WT_CIN, w=dict(wt_cin=40))
row("c3_wt_cin_below_cin", "conv_lif", EINVAL, WT_CIN, w=dict(wt_cin=32), g=dict(Cin=64))
row("c3_wt_cin_160", "conv_lif", EINVAL, WT_CIN, w=dict(wt_cin=160))
row("c3_wt_cin_then_negative", "conv_lif", EINVAL, WT_CIN, w=dict(wt_cin=40), T=-1)
row("c3_wt_cin_empty", "conv_lif", EINVAL, WT_CIN, w=dict(wt_cin=40), B=0)
row("c3_negative_t", "conv_lif", EINVAL, C3 + "negative T/B", T=-1)
row("c3_negative_b", "conv_lif", EINVAL, C3 + "negative T/B", B=-1)
row("c3_negative_b_t0", "conv_lif", EINVAL, C3 + "negative T/B", T=0, B=-1, x=None)
row("c3_negative_then_l", "conv_lif", EINVAL, C3 + "negative T/B", T=-1, w=dict(L=0.5))
row("c3_l", "conv_lif", EINVAL, L_MSG, w=dict(L=0.5))
row("c3_l_then_bn", "conv_lif", EINVAL, L_MSG, w=dict(L=0.5), bn=BADBN)
row("c3_l_empty", "conv_lif", EINVAL, L_MSG, w=dict(L=0.0), T=0)
row("c3_bn_null_mean", "conv_lif", EINVAL, BN_NULL, bn=dict(mean=None))
row("c3_bn_null_mul", "conv_lif", EINVAL, BN_NULL, bn=dict(mul=None))
row("c3_bn_null_bias", "conv_lif", EINVAL, BN_NULL, bn=dict(bias=None))
row("c3_bn_null_then_flags", "conv_lif", EINVAL, BN_NULL, bn=dict(bias=None, flags=0x7F3))
row("c3_bn_flags", "conv_lif", EINVAL, BN_FLAGS, bn=BADBN)
row("c3_bn_flags_empty", "conv_lif", EINVAL, BN_FLAGS, bn=BADBN, B=0)
row("c3_bn_then_cout_fire", "conv_lif", EINVAL, BN_FLAGS, bn=BADBN, w=dict(cout_fire=8))
row("c3_cout_fire_8", "conv_lif", EINVAL, C3 + "cout_fire 8 is not a multiple of 16 in (0, Cout = 32]",
    w=dict(cout_fire=8))
row("c3_cout_fire_48", "conv_lif", EINVAL, C3 + "cout_fire 48 is not a multiple of 16 in (0, Cout = 32]",
    w=dict(cout_fire=48))
row("c3_cout_fire_neg", "conv_lif", EINVAL, C3 + "cout_fire -16 is not a multiple of 16 in (0, Cout = 32]",
    w=dict(cout_fire=-16))
row("c3_cout_fire_empty", "conv_lif", EINVAL, C3 + "cout_fire 8 is not a multiple of 16 in (0, Cout = 32]",
    w=dict(cout_fire=8), T=0)
MANY = dict(H=4096, W=8192)                 # 1024 x 1024 patches of 4 x 8 pixels
row("c3_2_30_patches", "conv_lif", EUNSUP, C3 + "more than 2^30 patches in one launch", g=MANY, B=1024)
row("c3_2_30_patches_empty", "conv_lif", OK, None, g=MANY, B=1024, T=0)
F32_FRAMES = C3 + "float32 frames need x_flags and 8-byte aligned pixels"
row("c3_f32_x_unaligned", "conv_lif", EINVAL, F32_FRAMES, in_type=L.F32, g=dict(Cin=2), x_flags=P, x=P + 4,
    wt=None)
row("c3_f32_xs_t_odd", "conv_lif", EINVAL, F32_FRAMES, in_type=L.F32, g=dict(Cin=2), x_flags=P, xs_t=129)
row("c3_f32_xs_b_odd", "conv_lif", EINVAL, F32_FRAMES, in_type=L.F32, g=dict(Cin=2), x_flags=P, xs_b=513,
    impl=L.IMPL_MFMA)

# ---- snnqp_conv_lif_forward on its way to the direct-form kernel ---------------------------------------
EV_MSG = CL + "packed event frames need bit-packed spike output; unpack them first (%s)"
F32_MSG = (CL + "float32 input into integer codes is staged by the event-layer MFMA kernel only (%s); "
           "narrow it first (snnqp_narrow_f32 / snnqp_pack_bits_checked)")
POOL_MSG = CL + "the direct-form kernel does not fuse the max-pool; call snnqp_maxpool2x2 after it"
GEN = dict(impl=L.IMPL_GENERIC)
row("cg_ev1_generic", "conv_lif", EUNSUP, EV_MSG % "impl = GENERIC", "", in_type=L.EV1, g=dict(Cin=2), **GEN)
row("cg_ev4_why", "conv_lif", EUNSUP, EV_MSG % "spike output must be bit-packed", "", in_type=L.EV4,
    g=dict(Cin=2), s_type=L.F32)
row("cg_f32_generic", "conv_lif", EUNSUP, F32_MSG % "impl = GENERIC", "", in_type=L.F32, g=dict(Cin=2),
    x_flags=P, **GEN)
row("cg_f32_why", "conv_lif", EUNSUP, F32_MSG % "float32 input into integer codes needs Cin == 2", "",
    in_type=L.F32, x_flags=P)
row("cg_pool_generic", "conv_lif", EUNSUP, POOL_MSG, "", pool=2, **GEN)
row("cg_pool_why", "conv_lif", EUNSUP, POOL_MSG, "", pool=2, g=dict(stride_h=2))
row("cg_ev1_then_pool", "conv_lif", EUNSUP, EV_MSG % "impl = GENERIC", "", in_type=L.EV1, g=dict(Cin=2),
    pool=2, **GEN)
# the fallback is counted, with its reason, under IMPL_AUTO alone
row("cg_fallback_stride", "conv_lif", EINVAL, G_NULL, "conv: stride is not 1", g=dict(stride_h=2), x=None)
row("cg_fallback_no_wt", "conv_lif", EINVAL, G_NULL, "conv: MFMA-tiled codes `wt` not given", wt=None,
    s_out=None)
row("cg_fallback_f32_weights", "conv_lif", EINVAL, G_NULL, "conv: weights are not int8 codes",
    w=dict(wtype=L.W_F32), s_out=None)
row("cg_generic_no_fallback", "conv_lif", EINVAL, G_NULL, "", g=dict(stride_h=2), x=None, **GEN)
row("cg_generic_supported", "conv_lif", EINVAL, G_NULL, "", s_out=None, **GEN)

# ---- run_generic (the direct-form kernel), behind snnqp_conv_lif_forward with impl = GENERIC -------------
row("g_cin0", "conv_lif", EINVAL, "bad geometry H=8 W=8 Cin=0 Cout=32", g=dict(Cin=0), **GEN)
row("g_h_neg", "conv_lif", EINVAL, "bad geometry H=-1 W=8 Cin=32 Cout=32", g=dict(H=-1), **GEN)
row("g_cout0", "conv_lif", EINVAL, "bad geometry H=8 W=8 Cin=32 Cout=0", g=dict(Cout=0), **GEN)
row("g_groups0", "conv_lif", EINVAL, "in_features 32 / features 32 not divisible by feature_group_count 0",
    g=dict(groups=0), **GEN)
row("g_groups3", "conv_lif", EINVAL, "in_features 32 / features 32 not divisible by feature_group_count 3",
    g=dict(groups=3), **GEN)
row("g_stride0", "conv_lif", EINVAL, "conv_out_shape: non-positive stride/dilation/kernel", g=dict(stride_w=0),
    **GEN)
row("g_geometry_then_null", "conv_lif", EINVAL, "bad geometry H=8 W=8 Cin=0 Cout=32", g=dict(Cin=0), x=None,
    **GEN)
row("g_null_codes", "conv_lif", EINVAL, G_NULL, w=dict(w=None), **GEN)
row("g_null_x", "conv_lif", EINVAL, G_NULL, x=None, **GEN)
row("g_null_then_negative", "conv_lif", EINVAL, G_NULL, x=None, B=-1, **GEN)
row("g_negative_t", "conv_lif", EINVAL, "generic block: negative T/B", T=-1, **GEN)
row("g_negative_b", "conv_lif", EINVAL, "generic block: negative T/B", B=-1, x=None, T=0, **GEN)
row("g_empty_t", "conv_lif", OK, None, T=0, x=None, **GEN)
row("g_empty_b", "conv_lif", OK, None, B=0, s_out=None, **GEN)
row("g_empty_image", "conv_lif", OK, None, g=dict(H=0), **GEN)
row("g_empty_before_bn", "conv_lif", OK, None, T=0, bn=BADBN, w=dict(L=0.5), nrn=LIF0, **GEN)
row("g_lif_no_decay", "conv_lif", EINVAL, "LIF neuron needs a decay vector", nrn=LIF0, **GEN)
row("g_lif_then_bn", "conv_lif", EINVAL, "LIF neuron needs a decay vector", nrn=LIF0, bn=BADBN, **GEN)
row("g_bn_null", "conv_lif", EINVAL, BN_NULL, bn=dict(mul=None), **GEN)
row("g_bn_flags", "conv_lif", EINVAL, BN_FLAGS, bn=BADBN, **GEN)
row("g_bn_then_l", "conv_lif", EINVAL, BN_FLAGS, bn=BADBN, w=dict(L=0.5), **GEN)
row("g_bn_then_s_type", "conv_lif", EINVAL, BN_FLAGS, bn=BADBN, s_type=L.U8, **GEN)
row("g_s_type_u8", "conv_lif", EINVAL, "spike output type must be F32 or BITS", s_type=L.U8, **GEN)
row("g_s_type_then_input", "conv_lif", EINVAL, "spike output type must be F32 or BITS", s_type=7, in_type=7,
    **GEN)
row("g_int_in_type_7", "conv_lif", EUNSUP, INT_IN, in_type=7, **GEN)
row("g_int_in_type_7_auto", "conv_lif", EUNSUP, INT_IN,
    "conv: input must be BITS, U8, EV1, EV4 or (Cin == 2) F32", in_type=7)
row("g_input_then_l", "conv_lif", EUNSUP, INT_IN, in_type=7, w=dict(L=0.5), **GEN)
row("g_l", "conv_lif", EINVAL, L_MSG, w=dict(L=0.5), **GEN)
row("g_l_then_contraction", "conv_lif", EINVAL, L_MSG, w=dict(L=0.5), g=dict(Cin=8192), **GEN)
row("g_contraction", "conv_lif", EUNSUP, "contraction length 73728 overflows int32", g=dict(Cin=8192), **GEN)
row("g_weight_type_5", "conv_lif", EINVAL, "unknown weight type", w=dict(wtype=5), **GEN)
row("g_f32_weights_in_type_7", "conv_lif", EINVAL, "unknown input type 7", w=dict(wtype=L.W_F32), in_type=7,
    **GEN)

# ---- snnqp_conv_lif_forward_pred ---------------------------------------------------------------------
CP = "conv_lif_forward_pred: "
row("cp_null_pred", "conv_pred", EINVAL, CP + "null argument", pred=None)
row("cp_null_g", "conv_pred", EINVAL, CP + "null argument", g=None)
row("cp_null_nrn", "conv_pred", EINVAL, CP + "null argument", nrn=None)
row("cp_f32_no_flags", "conv_pred", EINVAL, CP + "float32 input into integer codes needs x_flags (snnqp.h)",
    in_type=L.F32)
row("cp_f32_no_flags_then_kind", "conv_pred", EINVAL,
    CP + "float32 input into integer codes needs x_flags (snnqp.h)", in_type=L.F32, nrn=dict(kind=9))
row("cp_kind", "conv_pred", EINVAL, CP + "unknown neuron kind 9", nrn=dict(kind=9))
row("cp_kind_then_pool", "conv_pred", EINVAL, CP + "unknown neuron kind -1", nrn=dict(kind=-1), pool=4)
row("cp_pool", "conv_pred", EINVAL, CP + "pool must be 1 or 2", pool=4)
row("cp_pool_then_format", "conv_pred", EINVAL, CP + "pool must be 1 or 2", pool=4, in_type=L.BITS)
FORMATS = CP + "byte, nibble or float32 frames (the event layer's own formats)"
row("cp_bits", "conv_pred", EUNSUP, FORMATS, in_type=L.BITS, g=dict(Cin=32), wt=P)
row("cp_ev1", "conv_pred", EUNSUP, FORMATS, in_type=L.EV1)
row("cp_format_then_geometry", "conv_pred", EUNSUP, FORMATS, in_type=L.EV1, g=dict(KH=5))
row("cp_why_cin", "conv_pred", EUNSUP, CP + "MFMA kernel: u8 input needs Cin == 2", g=dict(Cin=3))
row("cp_why_ev4", "conv_pred", EUNSUP, CP + "MFMA kernel: EV4 frames have Cin == 2", in_type=L.EV4,
    g=dict(Cin=4))
row("cp_why_stride", "conv_pred", EUNSUP, CP + "MFMA kernel: stride is not 1", g=dict(Cin=2, stride_w=3))
row("cp_why_lif", "conv_pred", EUNSUP, CP + "MFMA kernel: LIF without decay", nrn=LIF0)
row("cp_null_x", "conv_pred", EINVAL, C3 + "null pointer", x=None)
row("cp_null_then_negative", "conv_pred", EINVAL, C3 + "null pointer", s_out=None, T=-1)
row("cp_negative", "conv_pred", EINVAL, C3 + "negative T/B", B=-2)
row("cp_l", "conv_pred", EINVAL, L_MSG, w=dict(L=0.99))
row("cp_bn", "conv_pred", EINVAL, BN_FLAGS, bn=BADBN)
row("cp_cout_fire", "conv_pred", EINVAL, C3 + "cout_fire 24 is not a multiple of 16 in (0, Cout = 32]",
    w=dict(cout_fire=24))
row("cp_empty", "conv_pred", OK, None, T=0, x=None)
row("cp_f32_unaligned", "conv_pred", EINVAL, F32_FRAMES, in_type=L.F32, x_flags=P, x=P + 4)

# ---- snnqp_conv_lif_forward_if / snnqp_dense_lif_forward_if: the direct-form kernel, predicated ----------
CI = "conv_lif_forward_if: "
row("ci_null_pred", "conv_if", EINVAL, CI + "null argument", pred=None)
row("ci_null_w", "conv_if", EINVAL, CI + "null argument", w=None)
row("ci_kind", "conv_if", EINVAL, CI + "unknown neuron kind 0", nrn=dict(kind=0))
row("ci_kind_then_pool", "conv_if", EINVAL, CI + "unknown neuron kind 0", nrn=dict(kind=0), pool=0)
row("ci_pool", "conv_if", EINVAL, CI + "pool must be 1 or 2", pool=0)
row("ci_pool_then_geometry", "conv_if", EINVAL, CI + "pool must be 1 or 2", pool=3, g=dict(Cin=0))
row("ci_geometry", "conv_if", EINVAL, "bad geometry H=8 W=8 Cin=0 Cout=32", g=dict(Cin=0), pool=2)
row("ci_null_x_pool2", "conv_if", EINVAL, G_NULL, x=None, pool=2)
row("ci_negative", "conv_if", EINVAL, "generic block: negative T/B", T=-1, pool=2)
row("ci_empty_pool2", "conv_if", OK, None, T=0, x=None, pool=2)
row("ci_lif", "conv_if", EINVAL, "LIF neuron needs a decay vector", nrn=LIF0, pool=2)
row("ci_bn", "conv_if", EINVAL, BN_NULL, bn=dict(mean=None))
row("ci_f32_int8", "conv_if", EUNSUP, INT_IN, in_type=L.F32)
row("ci_l", "conv_if", EINVAL, L_MSG, w=dict(L=-1.0), pool=2)
DI = "dense_lif_forward_if: "
row("di_null_pred", "dense_if", EINVAL, DI + "bad argument", pred=None)
row("di_null_w", "dense_if", EINVAL, DI + "bad argument", w=None)
row("di_null_nrn", "dense_if", EINVAL, DI + "bad argument", nrn=None)
row("di_k0", "dense_if", EINVAL, DI + "bad argument", K=0)
row("di_n_neg", "dense_if", EINVAL, DI + "bad argument", N=-4)
row("di_kind", "dense_if", EINVAL, DI + "unknown neuron kind 5", nrn=dict(kind=5))
row("di_null_s_out", "dense_if", EINVAL, G_NULL, s_out=None)
row("di_negative", "dense_if", EINVAL, "generic block: negative T/B", B=-1)
row("di_empty", "dense_if", OK, None, B=0, x=None)
row("di_bn", "dense_if", EINVAL, BN_FLAGS, bn=BADBN)
row("di_s_type", "dense_if", EINVAL, "spike output type must be F32 or BITS", s_type=L.EV1)
row("di_f32_int8", "dense_if", EUNSUP, INT_IN, in_type=L.F32)
row("di_contraction", "dense_if", EUNSUP, "contraction length 70000 overflows int32", K=70000)

# ---- snnqp_dense_lif_forward / _ws: the entry checks ---------------------------------------------------
DL = "dense_lif_forward: "
D_FLAGS = DL + "float32 rows into integer codes need x_flags (snnqp.h)"
for entry in ("dense", "dense_ws"):
  row(entry + "_null_w", entry, EINVAL, DL + "null descriptor", w=None)
  row(entry + "_null_nrn", entry, EINVAL, DL + "null descriptor", nrn=None)
  row(entry + "_f32_no_flags", entry, EINVAL, D_FLAGS, in_type=L.F32, w=U8W)
  row(entry + "_f32_no_flags_then_kind", entry, EINVAL, D_FLAGS, in_type=L.F32, nrn=dict(kind=9), K=0)
  row(entry + "_k0", entry, EINVAL, DL + "bad K/N", K=0)
  row(entry + "_n0", entry, EINVAL, DL + "bad K/N", N=0)
  row(entry + "_k_then_kind", entry, EINVAL, DL + "bad K/N", K=-1, nrn=dict(kind=9))
  row(entry + "_kind", entry, EINVAL, DL + "unknown neuron kind 9", nrn=dict(kind=9))
  row(entry + "_kind_then_impl", entry, EINVAL, DL + "unknown neuron kind 0", nrn=dict(kind=0), impl=3)
  row(entry + "_impl", entry, EINVAL, DL + "unknown impl 3", impl=3)
  row(entry + "_impl_neg", entry, EINVAL, DL + "unknown impl -1", impl=-1, s_out=None)
  row(entry + "_null_s_out", entry, EINVAL, "dense mfma: null pointer", "", s_out=None)

# ---- the fp6 route: each condition of its predicate from both sides; the row drops s_out, and the ----
# ---- refusal names the kernel the call was routed to ---------------------------------------------------
F6 = "dense fp6: "
DM = "dense mfma: "
DW = "dense wide: "
NP = "null pointer"
T96 = "more than 96 (uint8 input: 64) timesteps (one sample must fit a row tile)"
REACH = "input strides beyond 32-bit word offsets within a workgroup"
row("f6_taken", "dense_ws", EINVAL, F6 + NP, "", w=FP6W, s_out=None)
row("f6_taken_plain_entry", "dense", EINVAL, F6 + NP, "", w=FP6W, s_out=None)
row("f6_taken_mfma", "dense_ws", EINVAL, F6 + NP, "", w=FP6W, s_out=None, impl=L.IMPL_MFMA)
row("f6_taken_wide_shape", "dense_ws", EINVAL, F6 + NP, "", w=FP6W, s_out=None, N=256)
row("f6_generic", "dense_ws", EINVAL, G_NULL, "", w=FP6W, s_out=None, **GEN)
row("f6_u8_input", "dense_ws", EINVAL, DM + NP, "", w=dict(FP6W, **U8W), s_out=None, in_type=L.U8, xs_t=64,
    xs_b=256)
row("f6_s_f32", "dense_ws", EINVAL, G_NULL, "dense: spike output must be bit-packed", w=FP6W, x=None,
    s_type=L.F32)
row("f6_f32_weights", "dense_ws", EINVAL, G_NULL, "dense: weights are not int8 codes",
    w=dict(FP6W, wtype=L.W_F32), s_out=None)
row("f6_no_tiles", "dense_ws", EINVAL, DM + NP, "", w=dict(code_max=7), s_out=None)
row("f6_code_max_0", "dense_ws", EINVAL, DM + NP, "", w=dict(FP6W, code_max=0), s_out=None)
row("f6_code_max_1", "dense_ws", EINVAL, F6 + NP, "", w=dict(FP6W, code_max=1), s_out=None)
row("f6_code_max_8", "dense_ws", EINVAL, DM + NP, "", w=dict(FP6W, code_max=8), s_out=None)
row("f6_code_max_8_wide", "dense_ws", EINVAL, DW + NP, "", w=dict(FP6W, code_max=8), s_out=None, N=256)
row("f6_t160", "dense_ws", EINVAL, F6 + NP, "", w=FP6W, s_out=None, T=160)
row("f6_t161", "dense_ws", EINVAL, G_NULL, "dense: " + T96, w=FP6W, s_out=None, T=161)
row("f6_t161_mfma", "dense_ws", EUNSUP, DL + "MFMA kernel: " + T96, "", w=FP6W, s_out=None, T=161,
    impl=L.IMPL_MFMA)
row("f6_k_exact", "dense_ws", EINVAL, F6 + NP, "", w=FP6W, s_out=None, K=2396745)      # 7 K = 2^24 - 1
row("f6_k_inexact", "dense_ws", EINVAL, DM + NP, "", w=FP6W, s_out=None, K=2396746)
row("f6_lif_no_decay", "dense_ws", EINVAL, G_NULL, "dense: LIF without decay", w=FP6W, s_out=None, nrn=LIF0)
row("f6_lif_decay", "dense_ws", EINVAL, F6 + NP, "", w=FP6W, s_out=None, nrn=dict(kind=L.NEURON_LIF, decay=P))
row("f6_plif", "dense_ws", EINVAL, F6 + NP, "", w=FP6W, s_out=None,
    nrn=dict(kind=L.NEURON_PARAMETRIC_LEAKY_IF))
row("f6_negative_xs_t", "dense_ws", EINVAL, G_NULL, "dense: " + REACH, w=FP6W, s_out=None, xs_t=-1)
row("f6_negative_xs_b", "dense_ws", EUNSUP, DL + "MFMA kernel: " + REACH, "", w=FP6W, s_out=None, xs_b=-8,
    impl=L.IMPL_MFMA)
# 160 samples of a workgroup: 3 xs_t + 160 xs_b + 2 words below 2^31
row("f6_reach_in", "dense_ws", EINVAL, F6 + NP, "", w=FP6W, s_out=None, xs_t=0, xs_b=13421772)
row("f6_reach_out", "dense_ws", EINVAL, DM + NP, "", w=FP6W, s_out=None, xs_t=0, xs_b=13421773)
row("f6_reach_t_in", "dense_ws", EINVAL, F6 + NP, "", w=FP6W, s_out=None, xs_t=715827882, xs_b=0, T=4, K=32)
row("f6_reach_t_out", "dense_ws", EINVAL, G_NULL, "dense: " + REACH, w=FP6W, s_out=None, xs_t=715827882,
    xs_b=0, T=4, K=64)
row("f6_reach_t0", "dense_ws", OK, None, w=FP6W, s_out=None, xs_t=1 << 40, T=0)
# run_dense_fp6
row("f6_null_x", "dense_ws", EINVAL, F6 + NP, w=FP6W, x=None)
row("f6_null_then_negative", "dense_ws", EINVAL, F6 + NP, w=FP6W, x=None, T=-1)
row("f6_negative_t", "dense_ws", EINVAL, F6 + "negative T/B", w=FP6W, T=-1)
row("f6_negative_b", "dense_ws", EINVAL, F6 + "negative T/B", w=FP6W, B=-1, T=0, x=None)
row("f6_negative_then_l", "dense_ws", EINVAL, F6 + "negative T/B", w=dict(FP6W, L=0.5), B=-1)
row("f6_l", "dense_ws", EINVAL, L_MSG, w=dict(FP6W, L=0.5))
row("f6_l_then_bn", "dense_ws", EINVAL, L_MSG, w=dict(FP6W, L=0.5), bn=BADBN)
row("f6_bn_null", "dense_ws", EINVAL, BN_NULL, w=FP6W, bn=dict(bias=None))
row("f6_bn_flags", "dense_ws", EINVAL, BN_FLAGS, w=FP6W, bn=BADBN)
row("f6_bn_empty", "dense_ws", EINVAL, BN_FLAGS, w=FP6W, bn=BADBN, T=0)
row("f6_empty_t", "dense_ws", OK, None, w=FP6W, T=0, x=None, s_out=None)
row("f6_empty_b", "dense_ws", OK, None, w=FP6W, B=0, s_out=None)

# ---- the wide route (more than 128 features): dense_wide_unsupported from both sides ---------------------
WIDE = dict(N=256, s_out=None)
U8IN = dict(in_type=L.U8, w=U8W, xs_t=64, xs_b=256)
F32IN = dict(in_type=L.F32, w=U8W, xs_t=64, xs_b=256, x_flags=P)
STAGED = (DL + "float32 rows into integer codes are staged by the wide MFMA kernel only (more than 128 "
          "features, T <= 64, K % 16 == 0, 16-byte aligned rows); narrow them first (snnqp_narrow_f32)")
MF = DL + "MFMA kernel: "
ALIGN = "uint8 rows not 16-byte aligned"
row("dw_taken", "dense_ws", EINVAL, DW + NP, "", **WIDE)
row("dw_taken_plain_entry", "dense", EINVAL, DW + NP, "", **WIDE)
row("dw_taken_mfma", "dense_ws", EINVAL, DW + NP, "", impl=L.IMPL_MFMA, **WIDE)
row("dw_taken_u8", "dense_ws", EINVAL, DW + NP, "", **dict(U8IN, **WIDE))
row("dw_taken_f32", "dense_ws", EINVAL, DW + NP, "", **dict(F32IN, **WIDE))
row("dw_generic", "dense_ws", EINVAL, G_NULL, "", **dict(WIDE, **GEN))
row("dw_n128", "dense_ws", EINVAL, DM + NP, "", N=128, s_out=None)
row("dw_n129", "dense_ws", EINVAL, DW + NP, "", N=129, s_out=None)
row("dw_t64", "dense_ws", EINVAL, DW + NP, "", T=64, **WIDE)
row("dw_t65", "dense_ws", EINVAL, DM + NP, "", T=65, **WIDE)
row("dw_t97", "dense_ws", EUNSUP, MF + T96, "", T=97, impl=L.IMPL_MFMA, **WIDE)
row("dw_f32_weights", "dense_ws", EUNSUP, MF + "weights are not int8 codes", "", w=dict(wtype=L.W_F32),
    impl=L.IMPL_MFMA, **WIDE)
row("dw_no_wt", "dense_ws", EINVAL, G_NULL, "dense: MFMA-tiled codes `wt` not given", wt=None, **WIDE)
row("dw_in_type", "dense_ws", EUNSUP, MF + "input must be bit-packed or uint8", "", in_type=L.EV1,
    impl=L.IMPL_MFMA, **WIDE)
row("dw_s_f32", "dense_ws", EUNSUP, MF + "spike output must be bit-packed", "", s_type=L.F32, N=256,
    impl=L.IMPL_MFMA)
row("dw_u8_no_col_sum", "dense_ws", EUNSUP, MF + "uint8 input needs snnqp_weight_t.col_sum", "",
    **dict(U8IN, w={}, impl=L.IMPL_MFMA, **WIDE))
row("dw_u8_k40", "dense_ws", EUNSUP, MF + "uint8 input needs K % 16 == 0", "",
    **dict(U8IN, K=40, impl=L.IMPL_MFMA, **WIDE))
row("dw_u8_k_large", "dense_ws", EUNSUP, MF + "uint8 input needs K <= 65536 (int32 accumulator)", "",
    **dict(U8IN, K=65552, impl=L.IMPL_MFMA, **WIDE))
row("dw_lif", "dense_ws", EUNSUP, MF + "LIF without decay", "", nrn=LIF0, impl=L.IMPL_MFMA, **WIDE)
row("dw_f32_no_col_sum", "dense_ws", EUNSUP, STAGED, "", **dict(F32IN, w={}, **WIDE))
row("dw_f32_k40", "dense_ws", EUNSUP, STAGED, "", **dict(F32IN, K=40, impl=L.IMPL_MFMA, **WIDE))
row("dw_f32_n64", "dense_ws", EUNSUP, STAGED, "", **dict(F32IN, s_out=None))
row("dw_f32_t65", "dense_ws", EUNSUP, STAGED, "", **dict(F32IN, T=65, **WIDE))
row("dw_f32_generic", "dense_ws", EUNSUP, STAGED, "", **dict(F32IN, **dict(WIDE, **GEN)))
row("dw_negative_xs_t", "dense_ws", EUNSUP, MF + REACH, "", xs_t=-2, impl=L.IMPL_MFMA, **WIDE)
row("dw_negative_xs_b", "dense_ws", EINVAL, G_NULL, "dense: " + REACH, xs_b=-8, **WIDE)
row("dw_u8_x_unaligned", "dense_ws", EUNSUP, MF + ALIGN, "", **dict(U8IN, x=P + 8, impl=L.IMPL_MFMA, **WIDE))
row("dw_u8_xs_t_unaligned", "dense_ws", EINVAL, G_NULL, "dense: " + ALIGN, **dict(U8IN, xs_t=72, **WIDE))
row("dw_u8_xs_b_unaligned", "dense_ws", EUNSUP, MF + ALIGN, "",
    **dict(U8IN, xs_b=264, impl=L.IMPL_MFMA, **WIDE))
row("dw_u8_unaligned_t65", "dense_ws", EUNSUP, MF + T96, "",
    **dict(U8IN, x=P + 8, T=65, impl=L.IMPL_MFMA, **WIDE))
row("dw_bits_any_alignment", "dense_ws", EINVAL, DW + NP, "", xs_t=3, xs_b=13, x=None, N=256)
row("dw_f32_x_unaligned", "dense_ws", EUNSUP, STAGED, "", **dict(F32IN, x=P + 4, **WIDE))
row("dw_f32_xs_t_unaligned", "dense_ws", EUNSUP, STAGED, "", **dict(F32IN, xs_t=66, **WIDE))
row("dw_f32_xs_b_unaligned", "dense_ws", EUNSUP, STAGED, "", **dict(F32IN, xs_b=257, **WIDE))
row("dw_f32_xs_4_aligned", "dense_ws", EINVAL, DW + NP, "", **dict(F32IN, xs_t=68, xs_b=260, **WIDE))
# 128 samples of a workgroup; a bit row is (K + 31) / 32 words, a uint8 or float32 row K elements
row("dw_reach_bits_in", "dense_ws", EINVAL, DW + NP, "", xs_t=0, xs_b=16777215, **WIDE)
row("dw_reach_bits_out", "dense_ws", EINVAL, DM + NP, "", xs_t=0, xs_b=16777216, **WIDE)
row("dw_reach_bits_k", "dense_ws", EINVAL, DW + NP, "", xs_t=0, xs_b=16777000, K=65536, **WIDE)
row("dw_reach_u8_in", "dense_ws", EINVAL, DW + NP, "", **dict(U8IN, xs_t=0, xs_b=16776688, K=65536, **WIDE))
row("dw_reach_u8_out", "dense_ws", EINVAL, DM + NP, "", **dict(U8IN, xs_t=0, xs_b=16776704, K=65536, **WIDE))
row("dw_reach_f32_in", "dense_ws", EINVAL, DW + NP, "", **dict(F32IN, xs_t=0, xs_b=4194300, **WIDE))
row("dw_reach_f32_out", "dense_ws", EUNSUP, STAGED, "", **dict(F32IN, xs_t=0, xs_b=4194304, **WIDE))
row("dw_reach_t", "dense_ws", EINVAL, G_NULL, "dense: " + REACH, xs_t=715827882, xs_b=0, **WIDE)
# the wide route counts T - 1 timestep strides as they come, the other two max(T - 1, 0): with no
# timestep, -xs_t brings a sample stride of 2^25 back in reach of the wide kernel, not of the 128-column one
row("dw_reach_t0_not_clamped", "dense_ws", OK, None, T=0, xs_t=1 << 33, xs_b=1 << 25, impl=L.IMPL_MFMA, **WIDE)
row("dm_reach_t0_clamped", "dense_ws", EUNSUP, MF + REACH, "", T=0, xs_t=1 << 33, xs_b=1 << 25,
    impl=L.IMPL_MFMA, s_out=None)
# run_dense_wide
WD = dict(N=256)
row("dw_null_x", "dense_ws", EINVAL, DW + NP, x=None, **WD)
row("dw_null_then_negative", "dense_ws", EINVAL, DW + NP, x=None, B=-1, **WD)
row("dw_negative_t", "dense_ws", EINVAL, DW + "negative T/B", T=-1, **WD)
row("dw_negative_b", "dense_ws", EINVAL, DW + "negative T/B", B=-1, T=0, **WIDE)
row("dw_negative_then_l", "dense_ws", EINVAL, DW + "negative T/B", T=-3, w=dict(L=0.5), **WD)
row("dw_l", "dense_ws", EINVAL, L_MSG, w=dict(L=0.5), **WD)
row("dw_l_then_bn", "dense_ws", EINVAL, L_MSG, w=dict(L=0.5), bn=BADBN, **WD)
row("dw_bn_null", "dense_ws", EINVAL, BN_NULL, bn=dict(mean=None), **WD)
row("dw_bn_flags", "dense_ws", EINVAL, BN_FLAGS, bn=BADBN, **WD)
row("dw_bn_empty", "dense_ws", EINVAL, BN_FLAGS, bn=BADBN, B=0, **WD)
row("dw_empty_t", "dense_ws", OK, None, T=0, **WIDE)
row("dw_empty_b", "dense_ws", OK, None, B=0, x=None, **WD)

# ---- the 128-column route: dense_mfma_unsupported and the row checks of the dispatch ---------------------
NARROW_U8 = dict(U8IN, s_out=None)
row("dm_f32_weights", "dense_ws", EUNSUP, MF + "weights are not int8 codes", "", w=dict(wtype=L.W_F32),
    impl=L.IMPL_MFMA)
row("dm_f32_weights_auto", "dense_ws", EINVAL, G_NULL, "dense: weights are not int8 codes",
    w=dict(wtype=L.W_F32), s_out=None, in_type=L.F32)
row("dm_no_wt", "dense_ws", EUNSUP, MF + "MFMA-tiled codes `wt` not given", "", wt=None, impl=L.IMPL_MFMA)
row("dm_no_wt_generic", "dense_ws", EINVAL, G_NULL, "", wt=None, s_out=None, **GEN)
row("dm_in_type", "dense_ws", EUNSUP, MF + "input must be bit-packed or uint8", "", in_type=L.EV4,
    impl=L.IMPL_MFMA)
row("dm_in_type_auto", "dense_ws", EUNSUP, INT_IN, "dense: input must be bit-packed or uint8", in_type=L.EV4)
row("dm_s_f32", "dense_ws", EUNSUP, MF + "spike output must be bit-packed", "", s_type=L.F32, impl=L.IMPL_MFMA)
row("dm_u8_no_col_sum", "dense_ws", EUNSUP, MF + "uint8 input needs snnqp_weight_t.col_sum", "",
    **dict(NARROW_U8, w={}, impl=L.IMPL_MFMA))
row("dm_u8_k40", "dense_ws", EINVAL, G_NULL, "dense: uint8 input needs K % 16 == 0", **dict(NARROW_U8, K=40))
row("dm_u8_k_large", "dense_ws", EUNSUP, MF + "uint8 input needs K <= 65536 (int32 accumulator)", "",
    **dict(NARROW_U8, K=65552, impl=L.IMPL_MFMA))
row("dm_lif", "dense_ws", EUNSUP, MF + "LIF without decay", "", nrn=LIF0, impl=L.IMPL_MFMA)
row("dm_wt_then_s_type", "dense_ws", EUNSUP, MF + "MFMA-tiled codes `wt` not given", "", wt=None,
    s_type=L.F32, impl=L.IMPL_MFMA)
row("dm_lif_then_t97", "dense_ws", EUNSUP, MF + "LIF without decay", "", nrn=LIF0, T=97, impl=L.IMPL_MFMA)
row("dm_t96", "dense_ws", EINVAL, DM + NP, "", T=96, s_out=None)
row("dm_t97", "dense_ws", EUNSUP, MF + T96, "", T=97, impl=L.IMPL_MFMA)
row("dm_t97_auto", "dense_ws", EINVAL, G_NULL, "dense: " + T96, T=97, s_out=None)
row("dm_u8_t64", "dense_ws", EINVAL, DM + NP, "", **dict(NARROW_U8, T=64))
row("dm_u8_t65", "dense_ws", EUNSUP, MF + T96, "", **dict(NARROW_U8, T=65, impl=L.IMPL_MFMA))
row("dm_u8_x_unaligned", "dense_ws", EUNSUP, MF + ALIGN, "", **dict(NARROW_U8, x=P + 1, impl=L.IMPL_MFMA))
row("dm_u8_xs_t_unaligned", "dense_ws", EUNSUP, MF + ALIGN, "", **dict(NARROW_U8, xs_t=8, impl=L.IMPL_MFMA))
row("dm_u8_xs_b_unaligned", "dense_ws", EINVAL, G_NULL, "dense: " + ALIGN, **dict(NARROW_U8, xs_b=250))
row("dm_u8_unaligned_t65", "dense_ws", EUNSUP, MF + T96, "",
    **dict(NARROW_U8, x=P + 1, T=65, impl=L.IMPL_MFMA))
row("dm_u8_unaligned_then_reach", "dense_ws", EUNSUP, MF + ALIGN, "",
    **dict(NARROW_U8, xs_t=-8, impl=L.IMPL_MFMA))
row("dm_negative_xs_t", "dense_ws", EUNSUP, MF + REACH, "", xs_t=-1, impl=L.IMPL_MFMA)
row("dm_negative_xs_b", "dense_ws", EUNSUP, MF + REACH, "", xs_b=-1, impl=L.IMPL_MFMA)
# 96 samples of a workgroup, and (K + 31) / 32 units of a row whatever the input type
row("dm_reach_in", "dense_ws", EINVAL, DM + NP, "", xs_t=0, xs_b=22369621, s_out=None)
row("dm_reach_out", "dense_ws", EUNSUP, MF + REACH, "", xs_t=0, xs_b=22369622, impl=L.IMPL_MFMA)
row("dm_reach_t", "dense_ws", EUNSUP, MF + REACH, "", xs_t=715827882, xs_b=0, impl=L.IMPL_MFMA)
row("dm_reach_u8_row_in_32s", "dense_ws", EINVAL, DM + NP, "",
    **dict(NARROW_U8, xs_t=0, xs_b=22369616, K=8192))
row("dm_reach_u8_out", "dense_ws", EUNSUP, MF + REACH, "",
    **dict(NARROW_U8, xs_t=0, xs_b=22369616, K=65536, impl=L.IMPL_MFMA))
# run_dense_mfma
row("dm_null_x", "dense_ws", EINVAL, DM + NP, x=None)
row("dm_null_then_negative", "dense_ws", EINVAL, DM + NP, x=None, T=-1)
row("dm_negative_t", "dense_ws", EINVAL, DM + "negative T/B", T=-1)
row("dm_negative_b", "dense", EINVAL, DM + "negative T/B", B=-1, T=0, x=None)
row("dm_negative_then_l", "dense_ws", EINVAL, DM + "negative T/B", T=-1, w=dict(L=0.5), bn=BADBN)
row("dm_l", "dense_ws", EINVAL, L_MSG, w=dict(L=0.5))
row("dm_l_then_bn", "dense", EINVAL, L_MSG, w=dict(L=0.5), bn=BADBN)
row("dm_bn_null", "dense_ws", EINVAL, BN_NULL, bn=dict(mul=None))
row("dm_bn_flags", "dense_ws", EINVAL, BN_FLAGS, bn=BADBN)
row("dm_bn_empty", "dense_ws", EINVAL, BN_FLAGS, bn=BADBN, T=0)
row("dm_empty_t", "dense_ws", OK, None, T=0, x=None)
row("dm_empty_b", "dense", OK, None, B=0, s_out=None)
# the direct form behind the dense entry point
row("dg_negative", "dense_ws", EINVAL, "generic block: negative T/B", "", T=-1, **GEN)
row("dg_empty", "dense_ws", OK, None, T=0, bn=BADBN, **GEN)
row("dg_bn", "dense_ws", EINVAL, BN_FLAGS, "", bn=BADBN, **GEN)
row("dg_l", "dense_ws", EINVAL, L_MSG, "", w=dict(L=0.5), **GEN)
row("dg_lif", "dense_ws", EINVAL, "LIF neuron needs a decay vector", "dense: LIF without decay", nrn=LIF0)

# ---- snnqp_dense_head_forward ----------------------------------------------------------------------
DH = "dense_head_forward: "
HU8 = dict(in_type=L.U8, w1=U8W, xs_t=64, xs_b=256)
HF32 = dict(in_type=L.F32, w1=U8W, xs_t=64, xs_b=256, x_flags=P)
row("dh_null_w1", "head", EINVAL, DH + "null argument", w1=None)
row("dh_null_w2", "head", EINVAL, DH + "null argument", w2=None)
row("dh_null_nrn1", "head", EINVAL, DH + "null argument", nrn1=None)
row("dh_null_nrn2", "head", EINVAL, DH + "null argument", nrn2=None)
row("dh_null_x", "head", EINVAL, DH + "null argument", x=None)
row("dh_null_logits", "head", EINVAL, DH + "null argument", logits=None)
row("dh_null_then_negative", "head", EINVAL, DH + "null argument", x=None, T=-1)
row("dh_negative_t", "head", EINVAL, DH + "bad sizes", T=-1)
row("dh_negative_b", "head", EINVAL, DH + "bad sizes", B=-1, T=0, x=None)
row("dh_k0", "head", EINVAL, DH + "bad sizes", K=0)
row("dh_n1_0", "head", EINVAL, DH + "bad sizes", N1=0)
row("dh_n2_0", "head", EINVAL, DH + "bad sizes", N2=0)
row("dh_group0", "head", EINVAL, DH + "bad sizes", group=0)
row("dh_sizes_then_group", "head", EINVAL, DH + "bad sizes", K=0, N2=21)
row("dh_n2_group", "head", EINVAL, DH + "N2=21 not divisible by group=2", N2=21)
row("dh_group_then_kind", "head", EINVAL, DH + "N2=20 not divisible by group=3", group=3, nrn1=dict(kind=0))
row("dh_kind1", "head", EINVAL, DH + "unknown neuron kind 0", nrn1=dict(kind=0))
row("dh_kind2", "head", EINVAL, DH + "unknown neuron kind 9", nrn2=dict(kind=9))
row("dh_kind_both", "head", EINVAL, DH + "unknown neuron kind 7", nrn1=dict(kind=7), nrn2=dict(kind=9))
row("dh_kind_then_l", "head", EINVAL, DH + "unknown neuron kind 9", nrn2=dict(kind=9), w1=dict(L=0.5))
row("dh_l1", "head", EINVAL, L_MSG, w1=dict(L=0.5))
row("dh_l2", "head", EINVAL, L_MSG, w2=dict(L=0.5))
row("dh_l_then_shape", "head", EINVAL, L_MSG, w2=dict(L=0.5), N1=513)
row("dh_l_empty", "head", EINVAL, L_MSG, w1=dict(L=0.5), B=0)
row("dh_n1_513", "head", EUNSUP, DH + "more than 512 hidden features", N1=513)
row("dh_n1_then_n2", "head", EUNSUP, DH + "more than 512 hidden features", N1=513, N2=130, T=65)
row("dh_n2_130", "head", EUNSUP, DH + "more than 128 output features", N2=130)
row("dh_n2_then_t", "head", EUNSUP, DH + "more than 128 output features", N2=130, T=0)
row("dh_t65", "head", EUNSUP, DH + "more than 64 timesteps", T=65)
row("dh_t0", "head", EUNSUP, DH + "no timestep", T=0, x=None)
row("dh_t0_b0", "head", EUNSUP, DH + "no timestep", T=0, B=0)
row("dh_t_then_block", "head", EUNSUP, DH + "more than 64 timesteps", T=65, wt1=None)
row("dh_w1_f32", "head", EUNSUP, DH + "weights are not int8 codes", w1=dict(wtype=L.W_F32))
row("dh_no_wt1", "head", EUNSUP, DH + "MFMA-tiled codes `wt` not given", wt1=None)
row("dh_in_type", "head", EUNSUP, DH + "input must be bit-packed or uint8", in_type=L.EV1)
row("dh_u8_no_col_sum", "head", EUNSUP, DH + "uint8 input needs snnqp_weight_t.col_sum", **dict(HU8, w1={}))
row("dh_f32_no_col_sum", "head", EUNSUP, DH + "uint8 input needs snnqp_weight_t.col_sum", **dict(HF32, w1={}))
row("dh_u8_k40", "head", EUNSUP, DH + "uint8 input needs K % 16 == 0", **dict(HU8, K=40))
row("dh_f32_k40", "head", EUNSUP, DH + "uint8 input needs K % 16 == 0", **dict(HF32, K=40))
row("dh_u8_k_large", "head", EUNSUP, DH + "uint8 input needs K <= 65536 (int32 accumulator)",
    **dict(HU8, K=65552))
row("dh_lif1", "head", EUNSUP, DH + "LIF without decay", nrn1=LIF0)
row("dh_block1_then_block2", "head", EUNSUP, DH + "LIF without decay", nrn1=LIF0, wt2=None)
row("dh_w2_f32", "head", EUNSUP, DH + "weights are not int8 codes", w2=dict(wtype=L.W_F32))
row("dh_no_wt2", "head", EUNSUP, DH + "MFMA-tiled codes `wt` not given", wt2=None)
row("dh_lif2", "head", EUNSUP, DH + "LIF without decay", nrn2=LIF0)
row("dh_block2_then_strides", "head", EUNSUP, DH + "MFMA-tiled codes `wt` not given", wt2=None, xs_t=-1)
row("dh_negative_xs_t", "head", EUNSUP, DH + "negative strides", xs_t=-1)
row("dh_negative_xs_b", "head", EUNSUP, DH + "negative strides", xs_b=-1)
row("dh_negative_then_unaligned", "head", EUNSUP, DH + "negative strides", **dict(HU8, xs_b=-1))
row("dh_u8_x_unaligned", "head", EUNSUP, DH + ALIGN, **dict(HU8, x=P + 4))
row("dh_u8_xs_t_unaligned", "head", EUNSUP, DH + ALIGN, **dict(HU8, xs_t=65))
row("dh_u8_xs_b_unaligned", "head", EUNSUP, DH + ALIGN, **dict(HU8, xs_b=260))
row("dh_f32_x_unaligned", "head", EUNSUP, DH + "float32 rows not 16-byte aligned", **dict(HF32, x=P + 8))
row("dh_f32_xs_t_unaligned", "head", EUNSUP, DH + "float32 rows not 16-byte aligned", **dict(HF32, xs_t=66))
row("dh_f32_xs_b_unaligned", "head", EUNSUP, DH + "float32 rows not 16-byte aligned", **dict(HF32, xs_b=258))
row("dh_f32_unaligned_then_flags", "head", EUNSUP, DH + "float32 rows not 16-byte aligned",
    **dict(HF32, xs_b=258, x_flags=None))
row("dh_f32_no_flags", "head", EUNSUP, DH + "float32 rows need x_flags", **dict(HF32, x_flags=None))
row("dh_f32_flags_then_reach", "head", EUNSUP, DH + "float32 rows need x_flags",
    **dict(HF32, x_flags=None, xs_b=1 << 30))
HREACH = DH + "input strides beyond 32-bit offsets within a workgroup"
# 128 samples; the head measures every row, a bit row too, as K units
row("dh_reach_bits_out", "head", EUNSUP, HREACH, xs_t=0, xs_b=16776704, K=65536)
row("dh_reach_bits_in_empty", "head", OK, None, xs_t=0, xs_b=16776703, K=65536, B=0)
row("dh_reach_u8_out", "head", EUNSUP, HREACH, **dict(HU8, xs_t=0, xs_b=16777216))
row("dh_reach_u8_in_empty", "head", OK, None, **dict(HU8, xs_t=0, xs_b=16777200, B=0))
row("dh_reach_f32_out", "head", EUNSUP, HREACH, **dict(HF32, xs_t=0, xs_b=4194304))
row("dh_reach_f32_in_empty", "head", OK, None, **dict(HF32, xs_t=0, xs_b=4194300, B=0))
row("dh_reach_t", "head", EUNSUP, HREACH, xs_t=715827882, xs_b=0)
row("dh_empty", "head", OK, None, B=0, x=None, logits=None)

# ---- snnqp_conv_forward / _ex / _if: the connection alone ---------------------------------------------
CF = "conv_forward: "
F32W = dict(wtype=L.W_F32)
row("cf_null_g", "conv_fwd", EINVAL, CF + "null geometry", g=None)
row("cf_nb_neg", "conv_fwd", EINVAL, CF + "bad NB", NB=-1)
row("cf_nb_2_31", "conv_fwd", EINVAL, CF + "bad NB", NB=1 << 31)
row("cf_null_w", "conv_fwd", EINVAL, G_NULL, w=None)
row("cf_null_x", "conv_fwd", EINVAL, G_NULL, x=None)
row("cf_null_y", "conv_fwd", EINVAL, G_NULL, y=None)
row("cf_null_x_f32_weights", "conv_fwd", EINVAL, G_NULL, x=None, w=F32W, in_type=L.F32)
row("cf_empty", "conv_fwd", OK, None, NB=0, x=None)
row("cf_geometry", "conv_fwd", EINVAL, "bad geometry H=8 W=8 Cin=32 Cout=-2", g=dict(Cout=-2))
row("cf_geometry_f32_gemm", "conv_fwd", EINVAL, "bad geometry H=8 W=8 Cin=0 Cout=32", g=dict(Cin=0), w=F32W,
    in_type=L.F32)
row("cf_groups_f32", "conv_fwd", EINVAL, "in_features 32 / features 32 not divisible by feature_group_count 3",
    g=dict(groups=3), w=F32W, in_type=L.F32)
row("cf_f32_int8", "conv_fwd", EUNSUP, INT_IN, in_type=L.F32)
row("cf_l", "conv_fwd", EINVAL, L_MSG, w=dict(L=0.5))
row("cf_contraction", "conv_fwd", EUNSUP, "contraction length 73728 overflows int32", g=dict(Cin=8192))
row("cf_weight_type", "conv_fwd", EINVAL, "unknown weight type", w=dict(wtype=3))
row("cf_f32_in_type_7", "conv_fwd", EINVAL, "unknown input type 7", w=F32W, in_type=7)
CX = "conv_forward_ex: "
CXM = CX + "MFMA kernel: "
MF_ = dict(impl=L.IMPL_MFMA)
row("cx_null_g", "conv_ex", EINVAL, CX + "null geometry", g=None)
row("cx_impl", "conv_ex", EINVAL, CX + "unknown impl 5", impl=5)
row("cx_impl_then_nb", "conv_ex", EINVAL, CX + "unknown impl 5", impl=5, NB=-1)
row("cx_nb", "conv_ex", EINVAL, CX + "bad NB", NB=-1)
row("cx_nb_generic", "conv_ex", EINVAL, CX + "bad NB", NB=1 << 31, **GEN)
row("cx_generic", "conv_ex", EINVAL, G_NULL, x=None, **GEN)
row("cx_null_w_mfma", "conv_ex", EUNSUP, CXM + "null weight descriptor", w=None, **MF_)
row("cx_null_w_auto", "conv_ex", EINVAL, G_NULL, w=None)
for name, why, change in [
    ("f32_weights", "weights are not int8 codes", dict(w=F32W)),
    ("kw5", "kernel is not 3x3", dict(g=dict(KW=5))),
    ("stride", "stride is not 1", dict(g=dict(stride_w=2))),
    ("pad", "padding is not ((1,1),(1,1))", dict(g=dict(pad_w_lo=0))),
    ("dilated", "dilated convolution", dict(g=dict(k_dil_h=3))),
    ("groups", "grouped convolution", dict(g=dict(groups=4))),
    ("w0", "empty image", dict(g=dict(W=0))),
    ("cout_neg", "no output channels", dict(g=dict(Cout=-1))),
    ("u8", "input must be bit-packed spikes", dict(in_type=L.U8)),
    ("cin0", "bit input needs Cin <= 128", dict(g=dict(Cin=0))),
    ("cin129", "bit input needs Cin <= 128", dict(g=dict(Cin=129))),
    ("no_wt", "MFMA-tiled codes `wt` not given", dict(wt=None)),
    ("wt_cin_40", "wt_cin must be a multiple of 32 in [Cin, 128]", dict(w=dict(wt_cin=40))),
    ("wt_cin_below", "wt_cin must be a multiple of 32 in [Cin, 128]", dict(w=dict(wt_cin=32), g=dict(Cin=33))),
    ("wt_cin_160", "wt_cin must be a multiple of 32 in [Cin, 128]", dict(w=dict(wt_cin=160))),
    ("2_30_patches", "2^30 patches or more in one launch", dict(g=MANY, NB=1024)),
    ("cout_then_input", "no output channels", dict(g=dict(Cout=0), in_type=L.U8)),
    ("input_then_cin", "input must be bit-packed spikes", dict(in_type=L.F32, g=dict(Cin=129))),
    ("wt_then_patches", "MFMA-tiled codes `wt` not given", dict(wt=None, g=MANY, NB=1024)),
]:
  row("cx_" + name, "conv_ex", EUNSUP, CXM + why, **dict(change, **MF_))
row("cx_auto_falls_back", "conv_ex", EINVAL, G_NULL, "", g=dict(stride_h=2), x=None)
row("cx_auto_no_wt", "conv_ex", EINVAL, G_NULL, "", wt=None, y=None)
row("cx_patches_empty", "conv_ex", OK, None, g=MANY, NB=0, **MF_)
CC = "conv3x3 currents: "
row("cc_null_codes", "conv_ex", EINVAL, CC + "null pointer", w=dict(w=None))
row("cc_null_x", "conv_ex", EINVAL, CC + "null pointer", x=None, **MF_)
row("cc_null_y", "conv_ex", EINVAL, CC + "null pointer", y=None)
row("cc_null_then_l", "conv_ex", EINVAL, CC + "null pointer", y=None, w=dict(L=0.5))
row("cc_null_codes_empty", "conv_ex", EINVAL, CC + "null pointer", w=dict(w=None), NB=0)
row("cc_l", "conv_ex", EINVAL, L_MSG, w=dict(L=0.5), **MF_)
row("cc_l_empty", "conv_ex", EINVAL, L_MSG, w=dict(L=0.5), NB=0)
row("cc_empty", "conv_ex", OK, None, NB=0, x=None, y=None)
CFI = "conv_forward_if: "
row("cfi_null_pred", "conv_fwd_if", EINVAL, CFI + "null argument", pred=None)
row("cfi_null_g", "conv_fwd_if", EINVAL, CFI + "null argument", g=None)
row("cfi_nb", "conv_fwd_if", EINVAL, CFI + "bad NB", NB=-1)
row("cfi_null_w", "conv_fwd_if", EINVAL, G_NULL, w=None)
row("cfi_null_y", "conv_fwd_if", EINVAL, G_NULL, y=None)
row("cfi_empty", "conv_fwd_if", OK, None, NB=0, x=None)
row("cfi_geometry", "conv_fwd_if", EINVAL, "conv_out_shape: non-positive stride/dilation/kernel",
    g=dict(KH=0))
row("cfi_f32_int8", "conv_fwd_if", EUNSUP, INT_IN, in_type=L.F32)
row("cfi_l", "conv_fwd_if", EINVAL, L_MSG, w=dict(L=0.5))

# ---- snnqp_conv3d_lif_forward -----------------------------------------------------------------------
C3D = "conv3d_lif_forward: "
row("c3d_null_g", "conv3d", EINVAL, "conv3d: null geometry", g3=None)
row("c3d_kd0", "conv3d", EINVAL, "conv3d: bad depth geometry", g3=dict(KD=0))
row("c3d_d_neg", "conv3d", EINVAL, "conv3d: bad depth geometry", g3=dict(D=-1))
row("c3d_stride0", "conv3d", EINVAL, "conv3d: bad depth geometry", g3=dict(stride=(0, 1, 1)))
row("c3d_pad_neg", "conv3d", EINVAL, "conv3d: bad depth geometry", g3=dict(pad_hi=(-1, 1, 1)))
row("c3d_depth_then_kind", "conv3d", EINVAL, "conv3d: bad depth geometry", g3=dict(KD=0), nrn=dict(kind=9))
row("c3d_kind_4", "conv3d", EINVAL, C3D + "unknown neuron kind 4", nrn=dict(kind=4))
row("c3d_kind_neg", "conv3d", EINVAL, C3D + "unknown neuron kind -1", nrn=dict(kind=-1), x=None)
row("c3d_geometry", "conv3d", EINVAL, "bad geometry H=8 W=8 Cin=32 Cout=0", g3=dict(Cout=0))
row("c3d_plane_stride0", "conv3d", EINVAL, "conv_out_shape: non-positive stride/dilation/kernel",
    g3=dict(stride=(1, 0, 1)))
row("c3d_null_w", "conv3d", EINVAL, G_NULL, w=None)
row("c3d_null_x", "conv3d", EINVAL, G_NULL, x=None)
row("c3d_null_x_no_neuron", "conv3d", EINVAL, G_NULL, x=None, nrn=None)
row("c3d_negative", "conv3d", EINVAL, "generic block: negative T/B", T=-1)
row("c3d_empty_t", "conv3d", OK, None, T=0, x=None)
row("c3d_empty_depth", "conv3d", OK, None, g3=dict(D=0, pad_lo=(0, 1, 1), pad_hi=(0, 1, 1)))
row("c3d_empty_depth_null_x", "conv3d", EINVAL, G_NULL, g3=dict(D=0, pad_lo=(0, 1, 1), pad_hi=(0, 1, 1)), x=None)
row("c3d_lif", "conv3d", EINVAL, "LIF neuron needs a decay vector", nrn=LIF0)
row("c3d_bn", "conv3d", EINVAL, BN_FLAGS, bn=BADBN)
row("c3d_s_type", "conv3d", EINVAL, "spike output type must be F32 or BITS", s_type=L.U8)
row("c3d_f32_int8", "conv3d", EUNSUP, INT_IN, in_type=L.F32)
row("c3d_l", "conv3d", EINVAL, L_MSG, w=dict(L=0.5), nrn=None, s_type=L.F32)
row("c3d_contraction", "conv3d", EUNSUP, "contraction length 69120 overflows int32",
    g3=dict(Cin=2560))                       # 3 x 3 x 3 x 2560: the depth taps count
row("c3d_weight_type", "conv3d", EINVAL, "unknown weight type", w=dict(wtype=2))

# ---- snnqp_conv_event_half_group and snnqp_conv_dequant_form: answers, no launch ------------------------
HG = "conv_event_half_group: "
row("hg_null_g", "half_group", EINVAL, HG + "null descriptor", g=None)
row("hg_null_w", "half_group", EINVAL, HG + "null descriptor", w=None)
row("hg_null_nrn", "half_group", EINVAL, HG + "null descriptor", nrn=None)
row("hg_kind", "half_group", EINVAL, HG + "unknown neuron kind 0", nrn=dict(kind=0))
row("hg_kind_then_pool", "half_group", EINVAL, HG + "unknown neuron kind 9", nrn=dict(kind=9), pool=0)
row("hg_pool", "half_group", EINVAL, HG + "pool must be 1 or 2", pool=0)
row("hg_pool_then_t", "half_group", EINVAL, HG + "pool must be 1 or 2", pool=3, T=-1)
row("hg_negative_t", "half_group", EINVAL, HG + "negative T", T=-1)
row("hg_l", "half_group", EINVAL, L_MSG, w=dict(L=0.5))
row("hg_l_then_cout_fire", "half_group", EINVAL, L_MSG, w=dict(L=0.5, cout_fire=8))
row("hg_cout_fire", "half_group", EINVAL,
    HG + "cout_fire 8 is not a multiple of 16 in (0, Cout = 32]", w=dict(cout_fire=8))
row("hg_cout_fire_large", "half_group", EINVAL,
    HG + "cout_fire 64 is not a multiple of 16 in (0, Cout = 32]", w=dict(cout_fire=64))
# (0 is SNNQP_OK: "no half group" -- not an event layer's launch, or one the kernel does not serve)
row("hg_u8_is_0", "half_group", 0, None, in_type=L.U8, w=dict(L=0.5))
row("hg_t0_is_0", "half_group", 0, None, T=0, w=dict(cout_fire=8))
row("hg_unsupported_is_0", "half_group", 0, None, g=dict(Cin=2, KH=5), w=dict(L=0.5))
row("hg_lif_no_decay_is_0", "half_group", 0, None, nrn=LIF0, w=dict(cout_fire=8))
row("hg_all_fire_is_0", "half_group", 0, None)
DF = "conv_dequant_form: "
row("df_null_w", "dequant_form", EINVAL, DF + "null descriptor", w=None)
row("df_null_nrn", "dequant_form", EINVAL, DF + "null descriptor", nrn=None)
row("df_f32_weights", "dequant_form", EINVAL, DF + "int8 codes only", w=F32W)

BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)

# ---- snnqp_dense_workspace_bytes(in_type, T, B, K, N, w): the byte count ------------------------------
# The base is a read-out the fp6 kernel splits along K (T = 20, B = 16, K = 32768, N = 128); every
# condition of the fp6 predicate that the size query repeats, and of the plan's own range, from both sides.
WS_BASE = dict(in_type=L.BITS, T=20, B=16, K=32768, N=128, w=FP6W)
WS_ROWS = [
    ("base", {}, 1052672),
    ("null_w", dict(w=None), 0),
    ("u8_input", dict(in_type=L.U8), 0),
    ("f32_weights", dict(w=dict(FP6W, wtype=L.W_F32)), 0),
    ("no_tiles", dict(w=dict(code_max=7)), 0),
    ("code_max_0", dict(w=dict(FP6W, code_max=0)), 0),
    ("code_max_1", dict(w=dict(FP6W, code_max=1)), 1052672),
    ("code_max_8", dict(w=dict(FP6W, code_max=8)), 0),
    ("k0", dict(K=0), 0),
    ("k_neg", dict(K=-5), 0),
    ("n0", dict(N=0), 0),
    ("n1", dict(N=1), 1052672),
    ("t0", dict(T=0), 0),
    ("t1", dict(T=1), 69632),
    ("t160", dict(T=160), 5246976),
    ("t161", dict(T=161), 0),
    ("b0", dict(B=0), 0),
    ("b1", dict(B=1), 69632),
    ("k_8191", dict(K=8191), 0),
    ("k_8192", dict(K=8192), 0),
    ("k_inexact_sums", dict(K=2396746), 1052672),       # the size query has no 7 K < 2^24 rule
    ("n_300", dict(N=300), 3149824),
    ("b_1024", dict(B=1024), 0),
]
