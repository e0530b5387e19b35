"""Thin functional layer: torch-ROCm tensors in, C-ABI calls (include/snnqp.h) out.

torch is plumbing here (device memory + the current HIP stream); every op below
is one call into libsnnqp.so.  Tensors must live on the GPU: there is no CPU
fallback and nothing in this package imports the oracle.
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L


# ---------------------------------------------------------------------------
# Packed spike tensors
# ---------------------------------------------------------------------------


class PackedSpikes:
  """Binary activations, channel-packed: `bits` is int32 [..., ceil(C/32)],
  channel c of a row in bit (c & 31) of word (c >> 5); `shape` is the logical
  shape [..., C] (time-major [T, B, ..., C] inside the model)."""

  def __init__(self, bits: torch.Tensor, channels: int):
    assert bits.dtype == torch.int32 and bits.is_contiguous()
    assert bits.shape[-1] == (channels + 31) // 32
    self.bits = bits
    self.channels = int(channels)
    # (C, H, W) when this is a [T, B, H*W*C] NHWC-ordered flattening of a
    # [T, B, H, W, C] block whose logical order is channel-major
    # (examples/tcja/models.py:189-190); consumers permute weight rows instead.
    self.flat_perm = None
    # ChannelMap when these are the computed channels of a compacted block: channel i
    # here is channel chan_map.index[i] of the block's logical output; the others never fire
    self.chan_map = None

  @property
  def shape(self):
    return tuple(self.bits.shape[:-1]) + (self.channels,)

  @property
  def device(self):
    return self.bits.device

  @property
  def ndim(self):
    return self.bits.ndim

  def __getitem__(self, idx):
    """Indexing over leading (non-channel) axes only."""
    if not isinstance(idx, tuple):
      idx = (idx,)
    assert len(idx) < self.bits.ndim, "cannot index the packed channel axis"
    out = PackedSpikes(self.bits[idx].contiguous(), self.channels)
    out.chan_map = self.chan_map
    return out

  def reshape_leading(self, *lead):
    out = PackedSpikes(self.bits.reshape(*lead, self.bits.shape[-1]), self.channels)
    out.chan_map = self.chan_map
    return out

  def swap_leading(self):
    """The two leading axes exchanged: [B, T, ...] <-> [T, B, ...]."""
    out = PackedSpikes(self.bits.transpose(0, 1).contiguous(), self.channels)
    out.chan_map = self.chan_map
    return out

  @staticmethod
  def cat_batch(parts):
    """Time-major rasters [T, b_i, ...] of one block joined along the batch axis."""
    first = parts[0]
    assert all(p.channels == first.channels and p.chan_map is first.chan_map for p in parts), \
        "rasters of different channel sets do not join"
    out = PackedSpikes(torch.cat([p.bits for p in parts], 1), first.channels)
    out.chan_map = first.chan_map
    return out

  def to_dense(self) -> torch.Tensor:
    return unpack_bits(self)

  def __repr__(self):
    return "PackedSpikes(shape=%s, device=%s)" % (self.shape, self.device)


class PackedFrames:
  """The model input -- 2-channel event frames [..., H, W, 2], leading axes [B, T] as the
  reference hands them over (examples/tcja/models.py:38, :109) -- in one of the wire
  formats of include/snnqp.h: `data` is int32 [..., ceil(H*W*2/32)] for _lib.EV1 (binary
  frames, 1 bit per element) or uint8 [..., H*W] for _lib.EV4 (counts <= 15, one byte per
  pixel).  What the host feed ships (feed.py): 1/8 resp. 1/2 of the uint8 bytes.  The
  first conv block stages EV1 frames directly; every other consumer unpacks."""

  def __init__(self, data: torch.Tensor, H: int, W: int, fmt: int):
    assert fmt in (L.EV1, L.EV4), fmt
    unit = frame_units(H, W, fmt)
    assert data.dtype == (torch.int32 if fmt == L.EV1 else torch.uint8), data.dtype
    assert data.shape[-1] == unit and data.is_contiguous(), (tuple(data.shape), unit)
    self.data, self.H, self.W, self.fmt = data, int(H), int(W), int(fmt)

  @property
  def shape(self):
    return tuple(self.data.shape[:-1]) + (self.H, self.W, 2)

  @property
  def device(self):
    return self.data.device

  @property
  def ndim(self):
    return self.data.ndim + 2

  @property
  def dtype(self):
    return torch.uint8

  @property
  def is_cuda(self):
    return self.data.is_cuda

  def __getitem__(self, idx):
    """Indexing over the leading (batch / time) axes only."""
    if not isinstance(idx, tuple):
      idx = (idx,)
    assert len(idx) < self.data.ndim, "cannot index inside a packed frame"
    return PackedFrames(self.data[idx].contiguous(), self.H, self.W, self.fmt)

  def narrow(self, dim, start, length):
    assert dim < self.data.ndim - 1
    return PackedFrames(self.data.narrow(dim, start, length).contiguous(), self.H, self.W, self.fmt)

  def to(self, device, non_blocking=False):
    return PackedFrames(self.data.to(device, non_blocking=non_blocking), self.H, self.W, self.fmt)

  def to_u8(self) -> torch.Tensor:
    return unpack_frames(self)

  def __repr__(self):
    return "PackedFrames(%s, shape=%s, device=%s)" % (
        "EV1" if self.fmt == L.EV1 else "EV4", self.shape, self.device)


class GatedSpikes:
  """gate[T, B, C] x spikes[T, B, H, W, C], NOT multiplied out: what a TCJA block hands to the next
  block (x_seq * out[:, :, None, None, :], examples/tcja/models.py:97).  A quantised 3x3 conv block
  contracts it in the 'gint' form (conv_gated_forward: the nine taps of a channel as an integer sum,
  the gates in one float32 chain); every other consumer multiplies it out (to_dense)."""

  def __init__(self, spikes: "PackedSpikes", gate: torch.Tensor, flat: bool = False):
    assert isinstance(spikes, PackedSpikes) and spikes.ndim == 5, "spikes [T, B, H, W, C], bit-packed"
    assert gate.dtype == torch.float32 and tuple(gate.shape) == (spikes.shape[0], spikes.shape[1], spikes.channels)
    self.spikes, self.gate = spikes, gate.contiguous()
    # flat: stands for the channel-major flattening [T, B, C H W] of the product (the transpose +
    # reshape of examples/tcja/models.py:189-190) -- nothing is moved, a dense block reads the
    # raster through its own weight layout (dense_gated_forward)
    self.flat = bool(flat)

  @property
  def shape(self):
    if self.flat:
      T, B, H, W, C = self.spikes.shape
      return (T, B, C * H * W)
    return self.spikes.shape

  @property
  def ndim(self):
    return 3 if self.flat else 5

  @property
  def device(self):
    return self.spikes.device

  def flattened(self) -> "GatedSpikes":
    return GatedSpikes(self.spikes, self.gate, flat=True)

  def to_dense(self) -> torch.Tensor:
    x = apply_gate(self.spikes, self.gate)
    if self.flat:
      x = x.permute(0, 1, 4, 2, 3)
      x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3] * x.shape[4]).contiguous()
    return x


class ChannelMap:
  """The channels a compacted block computes: `index` int64 [n], the logical output
  channel of computed channel i (live ones first, in their order, then silent ones as padding);
  `live` bool [n], which of them can fire; `full` the block's logical channel count."""

  def __init__(self, index, live, full: int):
    import numpy as np
    self.index = np.asarray(index, np.int64)
    self.live = np.asarray(live, bool)
    self.full = int(full)
    self._dev = {}

  def device_index(self, device) -> torch.Tensor:
    """int32 [n] on `device` (made once per device)."""
    key = str(device)
    t = self._dev.get(key)
    if t is None:
      t = self._dev[key] = torch.from_numpy(self.index.astype("int32")).to(device)
    return t

  def __repr__(self):
    return "ChannelMap(%d of %d, %d live)" % (self.index.size, self.full, int(self.live.sum()))


def scatter_spike_channels(s: "PackedSpikes", channel_map: torch.Tensor, cout: int) -> "PackedSpikes":
  """Bit-packed spikes [..., cin] -> [..., cout]: input channel c to output channel channel_map[c]
  (int32 device [cin]; entries outside [0, cout) dropped), every other channel zero
  (snnqp_scatter_spike_channels)."""
  bits = s.bits.contiguous()
  _require_gpu(bits, channel_map)
  assert channel_map.dtype == torch.int32 and channel_map.numel() == s.channels
  cw = (int(cout) + 31) // 32
  npix = bits.numel() // max(bits.shape[-1], 1) if bits.ndim else 0
  out = torch.empty(tuple(bits.shape[:-1]) + (cw,), dtype=torch.int32, device=bits.device)
  L.check(L.lib().snnqp_scatter_spike_channels(_ptr(bits), npix, s.channels,
                                                _ptr(channel_map.contiguous()), int(cout), _ptr(out),
                                                _stream()))
  return PackedSpikes(out, int(cout))


def truncate_silent_channels(x: "PackedSpikes"):
  """A compacted raster for a conv consumer: its channel count cut to the live channels rounded up
  to 16 (the K walk of the bit-input conv counts in 16s).  The map lists live
  channels first, so this drops silent padding only; the words per pixel stay as they are and the
  dropped bits are never set.  Returns (raster, its ChannelMap)."""
  cm = x.chan_map
  n = max(16, (int(cm.live.sum()) + 15) // 16 * 16)
  if n >= cm.index.size or (n + 31) // 32 != x.bits.shape[-1] or cm.live[n:].any():
    return x, cm
  cut = getattr(cm, "_cut16", None)
  if cut is None:
    cut = cm._cut16 = ChannelMap(cm.index[:n], cm.live[:n], cm.full)
  out = PackedSpikes(x.bits, n)
  out.chan_map = cut
  return out, cut


def expand_channels(x):
  """A compacted raster (PackedSpikes with a chan_map) at its logical width, channels in their
  original order, the ones not computed zero; anything else is returned as it is.  A flattened
  raster (flat_perm) is expanded as the [.., H, W, C] block it stands for and flattened again."""
  cm = getattr(x, "chan_map", None)
  if cm is None:
    return x
  flat = x.flat_perm
  if flat is not None:
    c, h, w = flat
    lead = tuple(x.bits.shape[:-1])
    blk = PackedSpikes(x.bits.reshape(*lead, h, w, c // 32).contiguous(), c)
    full = scatter_spike_channels(blk, cm.device_index(x.device), cm.full)
    out = PackedSpikes(full.bits.reshape(*lead, h * w * ((cm.full + 31) // 32)), h * w * cm.full)
    out.flat_perm = (cm.full, h, w)
    return out
  return scatter_spike_channels(x, cm.device_index(x.device), cm.full)


def frame_units(H: int, W: int, fmt: int) -> int:
  """Words (EV1) / bytes (EV4) of one packed frame."""
  return (H * W * 2 + 31) // 32 if fmt == L.EV1 else H * W


def pack_frames_host(x, fmt: int) -> PackedFrames:
  """uint8 frames [..., H, W, 2] in host memory (numpy array or CPU tensor) -> PackedFrames
  in host memory, with numpy -- what a data pipeline does once per sample before the feed.
  Raises if a value does not fit the format (EV1: > 1, EV4: > 15)."""
  import numpy as np
  a = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
  if a.dtype != np.uint8 or a.ndim < 3 or a.shape[-1] != 2:
    raise ValueError("event frames must be uint8 [..., H, W, 2], got %s %s" % (a.dtype, a.shape))
  H, W = a.shape[-3], a.shape[-2]
  lead = a.shape[:-3]
  limit = 1 if fmt == L.EV1 else 15
  if a.size and int(a.max()) > limit:
    raise ValueError("event count %d does not fit the %s frame format (max %d)"
                     % (int(a.max()), "EV1" if fmt == L.EV1 else "EV4", limit))
  if fmt == L.EV1:
    flat = np.ascontiguousarray(a).reshape(lead + (H * W * 2,))
    b = np.packbits(flat, axis=-1, bitorder="little")
    nbytes = frame_units(H, W, fmt) * 4
    if b.shape[-1] != nbytes:
      b = np.concatenate([b, np.zeros(lead + (nbytes - b.shape[-1],), np.uint8)], -1)
    data = torch.from_numpy(np.ascontiguousarray(b).view(np.int32))
  else:
    data = torch.from_numpy(np.ascontiguousarray(a[..., 0] | (a[..., 1] << 4)).reshape(lead + (H * W,)))
  return PackedFrames(data, H, W, fmt)


def pack_frames(x: torch.Tensor, fmt: int, flags: Optional[torch.Tensor] = None) -> PackedFrames:
  """uint8 frames [..., H, W, 2] on the GPU -> PackedFrames (snnqp_pack_frames).  Values the
  format cannot hold are saturated and flagged into the int32 device word `flags`
  (_lib.FLAG_GT_ONE / FLAG_GT_15) when one is given; nothing is read back here."""
  _require_gpu(x, flags)
  assert x.dtype == torch.uint8 and x.shape[-1] == 2 and x.ndim >= 3, (x.dtype, tuple(x.shape))
  x = x.contiguous()
  H, W = x.shape[-3], x.shape[-2]
  lead = tuple(x.shape[:-3])
  frames = math.prod(lead)
  data = torch.empty(lead + (frame_units(H, W, fmt),),
                     dtype=torch.int32 if fmt == L.EV1 else torch.uint8, device=x.device)
  L.check(L.lib().snnqp_pack_frames(_ptr(x), frames, H, W, fmt, _ptr(data), _ptr(flags), _stream()))
  return PackedFrames(data, H, W, fmt)


def pack_frames_checked(x: torch.Tensor) -> Tuple[PackedFrames, torch.Tensor]:
  """uint8 or float32 frames [..., H, W, 2] on the GPU -> (bit-packed EV1 frames, one int32 device
  word) in one pass (snnqp_pack_frames_checked): the word is zero iff every value is 0 or 1, i.e.
  iff the packed frames ARE the tensor -- the speculative half of conv_lif_forward(binary_first=True)."""
  _require_gpu(x)
  assert x.dtype in (torch.uint8, torch.float32) and x.shape[-1] == 2 and x.ndim >= 3, (x.dtype, tuple(x.shape))
  x = x.contiguous()
  H, W = x.shape[-3], x.shape[-2]
  lead = tuple(x.shape[:-3])
  frames = math.prod(lead)
  data = torch.empty(lead + (frame_units(H, W, L.EV1),), dtype=torch.int32, device=x.device)
  flags = torch.empty(1, dtype=torch.int32, device=x.device)
  L.check(L.lib().snnqp_pack_frames_checked(_ptr(x), L.U8 if x.dtype == torch.uint8 else L.F32, frames, H, W,
                                            _ptr(data), _ptr(flags), _stream()))
  return PackedFrames(data, H, W, L.EV1), flags


def unpack_frames(p: PackedFrames) -> torch.Tensor:
  """PackedFrames -> uint8 [..., H, W, 2] (snnqp_unpack_frames)."""
  _require_gpu(p.data)
  lead = tuple(p.data.shape[:-1])
  frames = math.prod(lead)
  y = torch.empty(lead + (p.H, p.W, 2), dtype=torch.uint8, device=p.device)
  L.check(L.lib().snnqp_unpack_frames(_ptr(p.data), p.fmt, frames, p.H, p.W, _ptr(y), _stream()))
  return y


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
  return None if t is None else ctypes.c_void_p(t.data_ptr())


def _require_gpu(*ts):
  for t in ts:
    if t is None:
      continue
    if not t.is_cuda:
      raise RuntimeError(
          "snnquantprune_amd ops run on the GPU only (tensor on %s); there is no "
          "CPU fallback" % t.device)


def _f32c(t: torch.Tensor) -> torch.Tensor:
  if t.dtype != torch.float32:
    t = t.to(torch.float32)
  return t.contiguous()


def _ref(st):
  """An optional ctypes struct by reference."""
  return None if st is None else ctypes.byref(st)


def _out_type(packed_out: bool) -> int:
  return L.BITS if packed_out else L.F32


def _bits_or_f32(x):
  """(tensor the kernel reads, its type, channels) of a PackedSpikes or a tensor taken as float32."""
  if isinstance(x, PackedSpikes):
    return x.bits, L.BITS, x.channels
  return _f32c(x), L.F32, x.shape[-1]


def is_pow2(x: float) -> bool:
  if not (x > 0) or math.isinf(x):
    return False
  m, _ = math.frexp(x)
  return m == 0.5


@dataclass
class Weight:
  """Kernel after the weight transforms (flax_qdense.py:74-85).

  wtype W_I8: `w` = int8 codes * mask in the reference's layout, current =
  fl(fl(acc / L) * m); `wt` = optional MFMA-tiled codes (pack_codes_mfma).
  wtype W_F32: `w` = float32 fake-quantised * mask kernel."""
  wtype: int
  w: torch.Tensor
  L: float = 1.0
  m: float = 1.0
  wt: Optional[torch.Tensor] = None
  abs_sum_max: int = 0      # |acc| <= abs_sum_max * x_max (max one-sided code sum over the outputs)
  code_max: int = 0         # max |code| (<= 7: exact in fp6)
  min_current_bits: int = 0  # smallest non-zero |BN(dequant(acc))| as float bits (current_min)
  col_sum: Optional[torch.Tensor] = None   # dense: int32 [N] column sums of the codes (uint8 input)
  wt6: Optional[torch.Tensor] = None       # dense, code_max <= 7: fp6 MFMA tiles (pack_codes_fp6)
  ch_stack_max: int = 0     # event layer: largest stacked per-channel code range (snnqp.h), 0 = unknown
  ch_slots: Optional[torch.Tensor] = None  # event layer: int32 [padded Cout] table slots (packing.table_slots)
  wt_cin: int = 0           # 3x3 conv over bits: the Cin `wt` is padded to (snnqp.h), 0 = 32 ceil(Cin / 32)
  cout_fire: int = 0        # event layer: output channels from here on never fire (snnqp.h), 0 = all may

  def struct(self) -> L.WeightT:
    # (built once per object: a Weight is not modified after the pack step made it --
    # dataclasses.replace makes a new one -- and it keeps its tensors alive)
    st = self.__dict__.get("_cstruct")
    if st is None:
      st = L.WeightT(self.wtype, self.w.data_ptr(), float(self.L), float(self.m),
                     int(self.abs_sum_max), int(self.code_max),
                     None if self.col_sum is None else self.col_sum.data_ptr(),
                     None if self.wt6 is None else self.wt6.data_ptr(),
                     int(self.min_current_bits), int(self.ch_stack_max),
                     None if self.ch_slots is None else self.ch_slots.data_ptr(), int(self.wt_cin),
                     int(self.cout_fire))
      self.__dict__["_cstruct"] = st
    return st

  @property
  def is_int(self):
    return self.wtype == L.W_I8


@dataclass
class Neuron:
  kind: int
  k: float = 2.0
  v_threshold: float = 1.0
  v_reset: float = 0.0
  decay: Optional[torch.Tensor] = None   # LIF: sigmoid(tau) per feature (device)

  def struct(self) -> L.NeuronT:
    return L.NeuronT(self.kind, float(self.k), float(self.v_threshold),
                     float(self.v_reset),
                     None if self.decay is None else self.decay.data_ptr())


@dataclass
class BnCoeffs:
  mean: torch.Tensor
  mul: torch.Tensor
  bias: torch.Tensor
  flags: int = 0      # _lib.BN_MEAN_ZERO | BN_BIAS_ZERO | BN_MUL_UNIFORM: known from the host-side fold

  def struct(self) -> L.BnT:
    return L.BnT(self.mean.data_ptr(), self.mul.data_ptr(), self.bias.data_ptr(), int(self.flags))


@dataclass
class ConvGeom:
  H: int
  W: int
  Cin: int
  Cout: int
  KH: int
  KW: int
  stride: Tuple[int, int] = (1, 1)
  pad: Tuple[Tuple[int, int], Tuple[int, int]] = ((0, 0), (0, 0))
  in_dil: Tuple[int, int] = (1, 1)
  k_dil: Tuple[int, int] = (1, 1)
  groups: int = 1

  def struct(self) -> L.ConvGeomT:
    return L.ConvGeomT(self.H, self.W, self.Cin, self.Cout, self.KH, self.KW,
                       self.stride[0], self.stride[1], self.pad[0][0],
                       self.pad[0][1], self.pad[1][0], self.pad[1][1],
                       self.in_dil[0], self.in_dil[1], self.k_dil[0],
                       self.k_dil[1], self.groups)

  def tag(self) -> str:
    return "%dx%dx%d->%d" % (self.H, self.W, self.Cin, self.Cout)

  def is_3x3_same(self) -> bool:
    """3x3, stride 1, pad 1, no dilation, one group: what the event layer and the gated conv serve."""
    return ((self.KH, self.KW) == (3, 3) and tuple(self.stride) == (1, 1)
            and tuple(map(tuple, self.pad)) == ((1, 1), (1, 1)) and tuple(self.in_dil) == (1, 1)
            and tuple(self.k_dil) == (1, 1) and self.groups == 1)

  def out_hw(self) -> Tuple[int, int]:
    oh, ow = ctypes.c_int32(), ctypes.c_int32()
    g = self.struct()
    L.check(L.lib().snnqp_conv_out_shape(ctypes.byref(g), ctypes.byref(oh),
                                         ctypes.byref(ow)))
    return oh.value, ow.value


@dataclass(frozen=True)
class Conv3dGeom:
  """Geometry of a 3-D QuantConv (snnqp_conv3d_geom_t): axis 0 = depth, 1 = height, 2 = width."""
  D: int
  H: int
  W: int
  Cin: int
  Cout: int
  KD: int
  KH: int
  KW: int
  stride: Tuple[int, int, int] = (1, 1, 1)
  pad: Tuple[Tuple[int, int], Tuple[int, int], Tuple[int, int]] = ((0, 0), (0, 0), (0, 0))
  in_dil: Tuple[int, int, int] = (1, 1, 1)
  k_dil: Tuple[int, int, int] = (1, 1, 1)
  groups: int = 1

  def struct(self) -> L.Conv3dGeomT:
    i3 = ctypes.c_int32 * 3
    return L.Conv3dGeomT(self.D, self.H, self.W, self.Cin, self.Cout, self.KD, self.KH, self.KW,
                         i3(*self.stride), i3(*[p[0] for p in self.pad]), i3(*[p[1] for p in self.pad]),
                         i3(*self.in_dil), i3(*self.k_dil), self.groups)

  def tag(self) -> str:
    return "%dx%dx%dx%d->%d" % (self.D, self.H, self.W, self.Cin, self.Cout)

  def out_dhw(self) -> Tuple[int, int, int]:
    od, oh, ow = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    g = self.struct()
    L.check(L.lib().snnqp_conv3d_out_shape(ctypes.byref(g), ctypes.byref(od), ctypes.byref(oh), ctypes.byref(ow)))
    return od.value, oh.value, ow.value


def _in_desc(x):
  """(pointer tensor, in_type, words/elements per pixel-row unit)."""
  if isinstance(x, PackedSpikes):
    return x.bits, L.BITS
  if isinstance(x, PackedFrames):
    return x.data, x.fmt
  if x.dtype == torch.uint8:
    return x, L.U8
  if x.dtype == torch.float32:
    return x, L.F32
  raise TypeError("activation dtype %s not supported (float32, uint8 or "
                  "PackedSpikes)" % x.dtype)


# ---------------------------------------------------------------------------
# weight transforms
# ---------------------------------------------------------------------------


def quantize(kind: int, w: torch.Tensor, mask: Optional[torch.Tensor], bits: int,
             p0: float, p1: float = 0.0, want_fq: bool = True,
             want_codes: bool = False, sign: bool = True):
  """snnqp_quantize_ex: returns (fq | None, codes | None, flags tensor | None); sign = False is
  the reference's unsigned form (levels 0 .. 2^bits - 1, quant.py:338-341)."""
  w = _f32c(w)
  _require_gpu(w, mask)
  if mask is not None:
    mask = _f32c(mask)
    assert mask.shape == w.shape
  fq = torch.empty_like(w) if want_fq else None
  codes = torch.empty(w.shape, dtype=torch.int8, device=w.device) if want_codes else None
  flags = torch.zeros(1, dtype=torch.int32, device=w.device) if (
      want_codes or mask is not None) else None
  L.check(L.lib().snnqp_quantize_ex(kind, _ptr(w), _ptr(mask), w.numel(), int(bits), 1 if sign else 0,
                                    float(p0), float(p1), _ptr(fq), _ptr(codes),
                                    _ptr(flags), _stream()))
  return fq, codes, flags


def pack_codes_mfma(codes: torch.Tensor, n_pad: Optional[int] = None) -> torch.Tensor:
  """[K, N] int8 codes -> MFMA B-operand tiles [Npad/32, K/32, 64, 16]."""
  _require_gpu(codes)
  assert codes.dtype == torch.int8
  c2 = codes.reshape(-1, codes.shape[-1]).contiguous()
  K, N = c2.shape
  n_pad = (N + 31) // 32 * 32 if n_pad is None else n_pad
  if K % 32:
    raise ValueError("MFMA tiling needs K % 32 == 0 (K = %d)" % K)
  wt = torch.empty((n_pad // 32, K // 32, 64, 16), dtype=torch.int8, device=codes.device)
  L.check(L.lib().snnqp_pack_codes_mfma(_ptr(c2), K, N, n_pad, _ptr(wt), _stream()))
  return wt


def pack_codes_fp6(codes: torch.Tensor, n_pad: Optional[int] = None) -> torch.Tensor:
  """[K, N] int8 codes of magnitude <= 7 -> fp6 MFMA tiles, uint8 [Npad/32, ceil(K/64), 1536]
  (snnqp_pack_codes_fp6): the packed form the f8f6f4 dense kernel streams."""
  _require_gpu(codes)
  assert codes.dtype == torch.int8
  c2 = codes.reshape(-1, codes.shape[-1]).contiguous()
  K, N = c2.shape
  n_pad = (N + 31) // 32 * 32 if n_pad is None else n_pad
  wt6 = torch.empty((n_pad // 32, (K + 63) // 64, 1536), dtype=torch.uint8, device=codes.device)
  L.check(L.lib().snnqp_pack_codes_fp6(_ptr(c2), K, N, n_pad, _ptr(wt6), _stream()))
  return wt6


# ---------------------------------------------------------------------------
# activation formats
# ---------------------------------------------------------------------------


class NotCapturable(RuntimeError):
  """The step needs a value on the host and is being recorded into a hipGraph, which cannot wait
  for one.  (Nothing in this package does any more -- float32 inputs are checked on the device,
  snnqp.h x_flags -- the class stays for callers that catch it.)"""


@dataclass
class FloatFallback:
  """What redoes an integer block whose float32 input turns out not to be integer-valued
  (the reference casts every input to float32, flax_qdense.py:67 / flax_qconv.py:101: a tensor of
  integers in [0, 255] takes the exact-integer kernels, anything else the float32 ones -- decided
  per tensor on the device, with no read-back: snnqp.h, x_flags and the *_if entry points).

  weight  the float32 fake-quantised kernel of the same layer (Weight, W_F32)
  x       the float32 tensor, when the integer launch reads a narrowed copy of it (narrow_f32_async /
          pack_bits_checked); None when the integer kernel stages the float32 tensor itself
  pred    the device word (int32 tensor of one element) the narrowing pass reported into; None when
          the integer kernel reports into a word of its own"""
  weight: "Weight"
  x: Optional[torch.Tensor] = None
  pred: Optional[torch.Tensor] = None


def forget_inputs():
  """Kept for callers of earlier versions (bench.py called it each step to drop cached facts about
  the last batch): nothing about an activation tensor is cached on the host any more."""


class CountHint:
  """What the first layer's kernel should size its tables for: the largest event count MOST of
  its staged chunks will hold on this device (1 = binary frames).  The kernel never trusts it
  -- it checks every chunk of input it stages and falls back per chunk (snnqp.h, x_max) -- and
  reports into `word` (eight int32 words: the largest value it saw and the number of chunks by
  their largest value, <= 1, 2, <= 7, <= 31, above, exactly 3); the words are copied back with a
  non-blocking copy and looked at on a later call, when the copy has long finished, so the host
  never waits for the device to learn about its input.

  The hint is the bucket bound that minimises the estimated time of the next launch: chunks
  within the hint run the table sized for it (the larger the table, the slower: COST), chunks
  above it the general path.  One hot pixel -- real DVS sensors have them -- therefore costs the
  few chunks that hold it, not the batch (a hint that followed the maximum would put every
  chunk on the slowest path)."""

  BOUNDS = (1, 2, 3, 7, 31)                 # the buckets' upper bounds; above 31: no table
  # relative time of a chunk in the table mode of a bound (headline layer, tools/conv0_hint_time.py:
  # per-channel tables 5.96 / 5.82 / 5.82 ms for hints 1 / 2 / 3, shared table 7.02) and on the
  # general path (x - 128, arithmetic: 10.9)
  COST = (1.0, 1.0, 1.0, 1.19, 1.19)
  GENERAL = 1.85

  def __init__(self, device):
    self.value = 1
    self.word = torch.zeros(8, dtype=torch.int32, device=device)
    self._host = torch.zeros(8, dtype=torch.int32).pin_memory()
    self._event = None
    self.max_seen = 0
    self.saw_counts = False      # a value above 1 has been reported on this device (sticky)

  def binary_so_far(self) -> bool:
    """Every launch that reported so far met binary frames only: byte / float32 frames are then
    worth packing to bits in front of the event layer (conv_lif_forward(binary_first=True)).
    Sticky the other way: one count above 1 -- a hot pixel -- and the frames go in as they are
    from then on, a failed speculation costs the batch twice."""
    return self.current() == 1 and not self.saw_counts

  @staticmethod
  def capturing() -> bool:
    """True while the current stream is being captured into a hipGraph: the read-back
    (a copy, a memset and an event) must stay out of the graph -- an event recorded on a
    capturing stream cannot be queried afterwards, and every replay would re-zero the
    shared word -- so a captured launch gets no `x_seen` word and the last known hint."""
    return torch.cuda.is_current_stream_capturing()

  @classmethod
  def choose(cls, words) -> int:
    """words = x_seen[1..6]: chunks with largest value <= 1, 2, <= 7, <= 31, above, and (part of
    the third) exactly 3 -> the hint."""
    w = list(words) + [0] * (6 - len(words))
    hist = [w[0], w[1], w[5], w[2] - w[5], w[3], w[4]]           # <= 1, 2, 3, 4..7, <= 31, above
    total = sum(hist)
    if total == 0:
      return 1
    best, best_cost = 255, cls.GENERAL * total          # no table fits: every chunk general
    below = 0
    for k, (bound, cost) in enumerate(zip(cls.BOUNDS, cls.COST)):
      below += hist[k]
      c = cost * below + cls.GENERAL * (total - below)
      if c < best_cost - 1e-9:
        best, best_cost = bound, c
    return best

  def current(self) -> int:
    if self.capturing():
      return self.value
    if self._event is not None and self._event.query():
      self._event = None
      words = [int(v) for v in self._host]
      self.max_seen = words[0]
      if self.max_seen > 1:
        self.saw_counts = True
      if sum(words[1:6]) > 0:
        # (never above what was seen: the tables are sized by abs_sum_max * hint, and a bucket
        # bound of 7 where the data stops at 4 can push 8-bit codes past the table's capacity)
        self.value = max(1, min(self.choose(words[1:7]), self.max_seen))
    return self.value

  def seen_word(self):
    """The device words a launch reports into, or None under graph capture."""
    return None if self.capturing() else self.word

  def launched(self):
    """After a launch that was given `word`: start its read-back (at most one in flight)."""
    if self.capturing():
      return
    if self._event is None:
      self._host.copy_(self.word, non_blocking=True)
      self.word.zero_()
      self._event = torch.cuda.Event()
      self._event.record()


_count_hints = {}


def count_hint(device) -> CountHint:
  key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
  h = _count_hints.get(key)
  if h is None:
    h = _count_hints[key] = CountHint(device)
  return h


def reset_count_hints(device=None):
  """Forget what the event layer has reported about its input on `device` (all devices: None): the
  next launch starts from "binary frames, nothing seen" again.  For a caller that switches to
  another data stream (bench.py between its legs); a model fed by one stream never needs it."""
  if device is None:
    _count_hints.clear()
  else:
    d = torch.device(device)
    _count_hints.pop(d.index if d.index is not None else torch.cuda.current_device(), None)


def f32_to_u8(x: torch.Tensor) -> torch.Tensor:
  x = _f32c(x)
  _require_gpu(x)
  y = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
  L.check(L.lib().snnqp_f32_to_u8(_ptr(x), _ptr(y), x.numel(), _stream()))
  return y


def narrow_f32_async(x: torch.Tensor):
  """float32 activations -> (uint8 copy, pred): one device pass (snnqp_narrow_f32) and NO
  read-back.  `pred` is a one-element int32 device tensor, non-zero when some element is not an
  integer in [0, 255] (the copy is then meaningless): the predicate of the float32 launch that
  follows the integer one (FloatFallback)."""
  x = _f32c(x)
  _require_gpu(x)
  y = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
  flags = torch.zeros(2, dtype=torch.int32, device=x.device)
  L.check(L.lib().snnqp_narrow_f32(_ptr(x), _ptr(y), x.numel(), _ptr(flags), _stream()))
  return y, flags[1:2]


def pack_bits_checked(x: torch.Tensor):
  """float32 / uint8 [..., C] -> (PackedSpikes, pred): `pred` (one int32 device word) is non-zero
  when some element is neither 0 nor 1 -- the raster then is not the tensor.  No read-back."""
  _require_gpu(x)
  if x.dtype not in (torch.float32, torch.uint8):
    x = x.to(torch.float32)
  x = x.contiguous()
  C = x.shape[-1]
  rows = x.numel() // C if C else 0
  bits = torch.empty(tuple(x.shape[:-1]) + ((C + 31) // 32,), dtype=torch.int32, device=x.device)
  flags = torch.zeros(1, dtype=torch.int32, device=x.device)
  L.check(L.lib().snnqp_pack_bits_checked(_ptr(x), L.F32 if x.dtype == torch.float32 else L.U8,
                                          rows, C, _ptr(bits), _ptr(flags), _stream()))
  return PackedSpikes(bits, C), flags


def pack_bits(x: torch.Tensor) -> PackedSpikes:
  """float32 / uint8 [..., C] (nonzero = spike) -> PackedSpikes."""
  _require_gpu(x)
  if x.dtype not in (torch.float32, torch.uint8):
    x = x.to(torch.float32)
  x = x.contiguous()
  C = x.shape[-1]
  rows = x.numel() // C if C else 0
  bits = torch.empty(tuple(x.shape[:-1]) + ((C + 31) // 32,), dtype=torch.int32,
                     device=x.device)
  L.check(L.lib().snnqp_pack_bits(_ptr(x), L.F32 if x.dtype == torch.float32 else L.U8,
                                  rows, C, _ptr(bits), _stream()))
  return PackedSpikes(bits, C)


def unpack_bits(s: PackedSpikes) -> torch.Tensor:
  _require_gpu(s.bits)
  y = torch.empty(s.shape, dtype=torch.float32, device=s.device)
  rows = y.numel() // s.channels
  L.check(L.lib().snnqp_unpack_bits(_ptr(s.bits), rows, s.channels, _ptr(y), _stream()))
  return y


# ---------------------------------------------------------------------------
# connection only
# ---------------------------------------------------------------------------


def fseq_gemm_supported(geom: ConvGeom) -> bool:
  """Shapes the float32-MFMA connection kernel serves (fseq_gemm.hip): stride 1, no
  dilation or groups, output size == input size (dense = 1x1 on a 1x1 image)."""
  (pt, pb), (pl, pr) = geom.pad
  return (geom.groups == 1 and tuple(geom.stride) == (1, 1) and tuple(geom.in_dil) == (1, 1)
          and tuple(geom.k_dil) == (1, 1)
          and pt + pb == geom.KH - 1 and pl + pr == geom.KW - 1)


_IMPLS = {"auto": L.IMPL_AUTO, "generic": L.IMPL_GENERIC, "mfma": L.IMPL_MFMA}


def conv_forward(x, geom: ConvGeom, weight: Weight, want_acc: bool = False, impl: str = "auto"):
  """x [NB, H, W, Cin] -> float32 [NB, OH, OW, Cout] (+ int32 accumulators).

  impl "auto": a 3x3 / stride 1 / pad 1 connection over PackedSpikes whose `weight` carries the
  MFMA-tiled codes `wt` runs on the currents form of the bit-input MFMA conv
  (snnqp_conv_forward_ex), where that kernel can serve it; everything else, and every Weight
  without `wt`, takes the launch of snnqp_conv_forward.  "generic": always that launch.  "mfma":
  the MFMA kernel or an error with the reason.  The results hold the same bits either way."""
  if impl not in _IMPLS:
    raise ValueError("impl must be 'auto', 'generic' or 'mfma', not %r" % (impl,))
  mfma = impl != "generic" and weight.wt is not None and isinstance(x, PackedSpikes)
  if impl == "mfma" and not mfma:
    raise L.SnnqpError(L.EUNSUPPORTED, "conv_forward: MFMA kernel: %s" % (
        "MFMA-tiled codes `wt` not given" if weight.wt is None else "input must be bit-packed spikes"))
  xt, in_type = _in_desc(x)
  xt = xt.contiguous()
  _require_gpu(xt, weight.w, weight.wt if mfma else None)
  NB = xt.shape[0]
  OH, OW = geom.out_hw()
  y = torch.empty((NB, OH, OW, geom.Cout), dtype=torch.float32, device=xt.device)
  acc = torch.empty(y.shape, dtype=torch.int32, device=xt.device) if want_acc else None
  g, w = geom.struct(), weight.struct()
  if mfma:
    L.check(L.lib().snnqp_conv_forward_ex(_ptr(xt), in_type, NB, ctypes.byref(g), ctypes.byref(w),
                                          _ptr(weight.wt), _ptr(y), _ptr(acc), _IMPLS[impl], _stream()))
  else:
    L.check(L.lib().snnqp_conv_forward(_ptr(xt), in_type, NB, ctypes.byref(g),
                                       ctypes.byref(w), _ptr(y), _ptr(acc), _stream()))
  return (y, acc) if want_acc else y


_IN_NAMES = {L.F32: "f32", L.U8: "u8", L.BITS: "bits"}


def conv_float_form(x, geom: ConvGeom, weight: Weight, NB: Optional[int] = None):
  """Which kernel conv_forward(x, geom, weight) runs on the launch of snnqp_conv_forward
  (snnqp_conv_float_form; no device work, host tensors serve as well): "direct" for the direct-form
  kernel, else (input type "f32" / "u8" / "bits", staging mode 0..3, tile 64 or 128) of the
  float32-MFMA connection, e.g. ("u8", 3, 128).  `x`: the contiguous [NB, H, W, Cin] tensor or
  PackedSpikes as the library would get it -- only its address, type and NB count --, or a pair
  (address, in_type) with `NB` given, where no tensor exists."""
  if isinstance(x, tuple):
    addr, in_type = int(x[0]), int(x[1])
    if NB is None:
      raise ValueError("conv_float_form: an (address, in_type) pair needs NB")
  else:
    xt, in_type = _in_desc(x)
    if not xt.is_contiguous():
      raise ValueError("conv_float_form: x must be contiguous (its address decides)")
    addr = xt.data_ptr()
    NB = xt.shape[0] if NB is None else NB
  g, w = geom.struct(), weight.struct()
  rc = L.lib().snnqp_conv_float_form(ctypes.c_void_p(addr), in_type, int(NB), ctypes.byref(g), ctypes.byref(w))
  if rc < 0:
    L.check(rc)
  if rc == 0:
    return "direct"
  return _IN_NAMES[in_type], rc & 3, rc & ~3


def conv3d_lif_forward(x, geom: Conv3dGeom, weight: Weight, neuron: Optional[Neuron] = None,
                       bn: Optional[BnCoeffs] = None, u0: Optional[torch.Tensor] = None, want_u: bool = True,
                       packed_out: bool = False, pred: Optional[torch.Tensor] = None, out=None):
  """3-D QuantConv (snnqp_conv3d_lif_forward).  With a neuron: x [T, B, D, H, W, Cin] ->
  (u_T [B, OD, OH, OW, Cout] | None, spikes [T, B, OD, OH, OW, Cout]); without: x [NB, D, H, W, Cin]
  -> float32 currents [NB, OD, OH, OW, Cout].  pred / out: the predicated second launch of a
  speculative pair writes into the outputs `out` of the first, only if *pred != 0."""
  xt, in_type = _in_desc(x)
  xt = xt.contiguous()
  _require_gpu(xt, weight.w, u0)
  OD, OH, OW = geom.out_dhw()
  dev = xt.device
  unit = geom.D * geom.H * geom.W * xt.shape[-1]
  g, w = geom.struct(), weight.struct()
  b = bn.struct() if bn is not None else None
  if neuron is None:
    NB = xt.shape[0]
    y = out if out is not None else torch.empty((NB, OD, OH, OW, geom.Cout), dtype=torch.float32, device=dev)
    with _timed("conv3d[%s]" % geom.tag()):
      L.check(L.lib().snnqp_conv3d_lif_forward(_ptr(pred), _ptr(xt), in_type, 0, unit, 1, NB, ctypes.byref(g),
                                               ctypes.byref(w), None, None, None, None, _ptr(y), L.F32, _stream()))
    return y
  T, B = xt.shape[0], xt.shape[1]
  u0, u_out, s, spikes = _scan_outputs(dev, (T, B, OD, OH, OW), geom.Cout, u0, want_u, packed_out, out=out)
  n = neuron.struct()
  with _timed("conv3d[%s]" % geom.tag()):
    L.check(L.lib().snnqp_conv3d_lif_forward(_ptr(pred), _ptr(xt), in_type, B * unit, unit, T, B, ctypes.byref(g),
                                             ctypes.byref(w), _ref(b),
                                             ctypes.byref(n), _ptr(u0), _ptr(u_out), _ptr(s),
                                             _out_type(packed_out), _stream()))
  return u_out, spikes


def conv_forward_speculative(x: torch.Tensor, geom: ConvGeom, int_weight: Weight, float_weight: Weight):
  """The connection alone on a float32 tensor [NB, H, W, Cin] that MAY hold integers in [0, 255]
  (QuantDense / QuantConv called outside a SpikingBlock): narrowed to uint8 and checked in one
  device pass, the integer connection on the copy, then the float32 connection into the same
  output, executed only if the check failed (snnqp_conv_forward_if).  Nothing is read back."""
  x = _f32c(x)
  x8, pred = narrow_f32_async(x)
  y = conv_forward(x8, geom, int_weight)
  g, w = geom.struct(), float_weight.struct()
  L.check(L.lib().snnqp_conv_forward_if(_ptr(pred), _ptr(x), L.F32, x.shape[0], ctypes.byref(g), ctypes.byref(w),
                                        _ptr(y), _stream()))
  return y


def _pack_gated(codes: torch.Tensor, code_max: int, bytes_fn, pack_fn, *dims) -> torch.Tensor:
  """bytes_fn(C, N, code_max) bytes, filled by pack_fn(codes, *dims, code_max, out, stream); dims = (C, ..., N)"""
  codes = codes.contiguous()
  out = torch.empty(int(bytes_fn(dims[0], dims[-1], int(code_max))), dtype=torch.uint8, device=codes.device)
  L.check(pack_fn(_ptr(codes), *dims, int(code_max), _ptr(out), _stream()))
  return out


def pack_codes_gated(codes: torch.Tensor, code_max: int = 7) -> torch.Tensor:
  """int8 HWIO codes [3, 3, Cin, Cout] -> the operand layout of conv_gated_forward
  (snnqp_pack_codes_gated_ex): e2m3 for code_max <= 7, two e3m2 digits per code up to 127."""
  _require_gpu(codes)
  assert codes.dtype == torch.int8 and codes.ndim == 4 and tuple(codes.shape[:2]) == (3, 3)
  return _pack_gated(codes, code_max, L.lib().snnqp_conv_gated_packed_bytes_ex, L.lib().snnqp_pack_codes_gated_ex,
                     codes.shape[2], codes.shape[3])


def conv_gated_forward(x: GatedSpikes, geom: ConvGeom, weight: Weight, packed: torch.Tensor) -> torch.Tensor:
  """gate x raster [T, B, H, W, Cin] -> float32 currents [T, B, H, W, Cout] in the 'gint' form
  (snnqp_conv_gated_forward); raises SnnqpError(EUNSUPPORTED) for shapes it does not serve."""
  bits, gate = x.spikes.bits.contiguous(), x.gate
  _require_gpu(bits, gate, weight.w, packed)
  T, B, H, W, _ = x.shape
  assert (H, W, x.spikes.channels) == (geom.H, geom.W, geom.Cin), (x.shape, geom)
  y = torch.empty((T, B, H, W, geom.Cout), dtype=torch.float32, device=bits.device)
  g, w = geom.struct(), weight.struct()
  with _timed("conv[gated %s]" % geom.tag()):
    L.check(L.lib().snnqp_conv_gated_forward(_ptr(bits), _ptr(gate), T * B, ctypes.byref(g), ctypes.byref(w),
                                             _ptr(packed), _ptr(y), _stream()))
  return y


def pack_codes_dense_gated(codes: torch.Tensor, C: int, HW: int, code_max: int = 7) -> torch.Tensor:
  """int8 codes [C * HW, N] (rows channel-major) -> the operand layout of dense_gated_forward
  (snnqp_pack_codes_dense_gated_ex): e2m3 for code_max <= 7, two e3m2 digits per code up to 127."""
  _require_gpu(codes)
  assert codes.dtype == torch.int8 and codes.ndim == 2 and codes.shape[0] == C * HW
  return _pack_gated(codes, code_max, L.lib().snnqp_dense_gated_packed_bytes_ex,
                     L.lib().snnqp_pack_codes_dense_gated_ex, C, HW, codes.shape[1])


def dense_gated_forward(x: GatedSpikes, weight: Weight, packed: torch.Tensor) -> torch.Tensor:
  """channel-major flattening of gate x raster [T, B, (C, H, W)] -> float32 currents [T, B, N] in
  the 'gint' form (snnqp_dense_gated_forward); raises SnnqpError(EUNSUPPORTED) for shapes it does
  not serve."""
  bits, gate = x.spikes.bits.contiguous(), x.gate
  _require_gpu(bits, gate, weight.w, packed)
  T, B, H, W, C = x.spikes.shape
  N = weight.w.shape[-1]
  assert weight.w.shape[0] == C * H * W, (tuple(weight.w.shape), x.spikes.shape)
  y = torch.empty((T, B, N), dtype=torch.float32, device=bits.device)
  w = weight.struct()
  with _timed("dense[gated K=%d N=%d]" % (C * H * W, N)):
    L.check(L.lib().snnqp_dense_gated_forward(_ptr(bits), _ptr(gate), T * B, H * W, C, N, ctypes.byref(w),
                                              _ptr(packed), _ptr(y), _stream()))
  return y


def conv_gated_plan(cout: int, code_max: int) -> Tuple[int, int, bool]:
  """(full_groups, rest_tiles, wide) of conv_gated_forward for `cout` outputs and codes up to
  `code_max` (snnqp_conv_gated_plan; no device work): a launch of `full_groups` workgroup rows with
  four output tiles of 32 each, then one with the last `rest_tiles` tiles; wide = the two-digit
  e3m2 layout.  Raises SnnqpError(EINVAL) for cout < 1 or code_max outside 1..127."""
  full, rest, wide = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
  L.check(L.lib().snnqp_conv_gated_plan(int(cout), int(code_max), ctypes.byref(full), ctypes.byref(rest),
                                        ctypes.byref(wide)))
  return full.value, rest.value, bool(wide.value)


def dense_gated_plan(n: int, code_max: int) -> Tuple[int, bool]:
  """(grid_y, wide) of dense_gated_forward for `n` outputs and codes up to `code_max`
  (snnqp_dense_gated_plan; no device work): workgroups of up to 512 outputs per 32 images."""
  gy, wide = ctypes.c_int32(), ctypes.c_int32()
  L.check(L.lib().snnqp_dense_gated_plan(int(n), int(code_max), ctypes.byref(gy), ctypes.byref(wide)))
  return gy.value, bool(wide.value)


def dense_wide_plan(T: int, B: int, N: int, fused: bool = True, may_split: bool = True) -> Tuple[int, int, int, int]:
  """(rt, ct, sph, csplit) of the wide dense kernel (snnqp_dense_wide_plan; no device work): the
  fused head (dense_head_forward, N = its hidden width) or the stand-alone wide block; may_split =
  the head has its workspace."""
  rt, ct, sph, cs = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
  L.check(L.lib().snnqp_dense_wide_plan(int(T), int(B), int(N), int(bool(fused)), int(bool(may_split)),
                                        ctypes.byref(rt), ctypes.byref(ct), ctypes.byref(sph), ctypes.byref(cs)))
  return rt.value, ct.value, sph.value, cs.value


def dense_fp6_plan(T: int, B: int, K: int, N: int, ws: Optional[int] = None,
                   ws_bytes: int = 0) -> Tuple[int, int, int, int]:
  """(rt, ks, gx, gcz) of the fp4 x fp6 dense launch with the workspace at ADDRESS `ws` (None: no
  workspace) of `ws_bytes` bytes (snnqp_dense_fp6_plan; no device work, the address is not read)."""
  rt, ks, gx, gcz = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
  L.check(L.lib().snnqp_dense_fp6_plan(int(T), int(B), int(K), int(N), None if ws is None else ctypes.c_void_p(ws),
                                       int(ws_bytes), ctypes.byref(rt), ctypes.byref(ks), ctypes.byref(gx),
                                       ctypes.byref(gcz)))
  return rt.value, ks.value, gx.value, gcz.value


def dense_mfma_plan(in_type: int, T: int, B: int, N: int) -> Tuple[int, int, int, int]:
  """(rt, sb, gx, gy) of the int8 128-column dense launch on rows of `in_type` (L.BITS or L.U8):
  snnqp_dense_mfma_plan, the SNNQP_DENSE_MFMA_RT knob included; no device work."""
  rt, sb, gx, gy = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
  L.check(L.lib().snnqp_dense_mfma_plan(int(in_type), int(T), int(B), int(N), ctypes.byref(rt), ctypes.byref(sb),
                                        ctypes.byref(gx), ctypes.byref(gy)))
  return rt.value, sb.value, gx.value, gy.value


# ---------------------------------------------------------------------------
# per-launch timing with HIP events on the launch stream (bench.py roofline)
# ---------------------------------------------------------------------------

_PROFILE = None
PROFILE_NOTES = {}      # tag -> facts about the launches of the last profiled region


def profile_start():
  global _PROFILE
  _PROFILE = {}
  PROFILE_NOTES.clear()


def profile_stop():
  """{tag: (launches, total milliseconds)} since profile_start()."""
  global _PROFILE
  prof, _PROFILE = _PROFILE or {}, None
  torch.cuda.synchronize()
  return {tag: (len(evs), sum(a.elapsed_time(b) for a, b in evs))
          for tag, evs in prof.items()}


class _timed:
  def __init__(self, tag):
    self.tag = tag

  def __enter__(self):
    if _PROFILE is not None:
      self.a = torch.cuda.Event(enable_timing=True)
      self.b = torch.cuda.Event(enable_timing=True)
      self.a.record()

  def __exit__(self, *exc):
    if _PROFILE is not None and exc[0] is None:
      self.b.record()
      _PROFILE.setdefault(self.tag, []).append((self.a, self.b))
    return False


# ---------------------------------------------------------------------------
# fused SpikingBlock
# ---------------------------------------------------------------------------


_current_min_cache = None


def current_min_bits(weight: Weight, bn: Optional[BnCoeffs], bound: int, cout: int) -> int:
  """float32 bits of the smallest non-zero |BatchNorm(dequant(acc))| over |acc| <= bound and
  the channels: what Weight.min_current_bits wants (one device pass + a 4-byte read-back per
  (weights, BatchNorm) version, cached)."""
  global _current_min_cache
  if _current_min_cache is None:
    from ._cache import TensorCache
    _current_min_cache = TensorCache(64)
  key = (weight.w,) + ((bn.mean, bn.mul, bn.bias) if bn is not None else (None, None, None))
  extra = (int(bound), int(cout), float(weight.L), float(weight.m))
  v = _current_min_cache.get(key, extra)
  if v is None:
    _require_gpu(weight.w)
    out = torch.full((1,), 0x7F800000, dtype=torch.int32, device=weight.w.device)
    w = weight.struct()
    b = bn.struct() if bn is not None else None
    L.check(L.lib().snnqp_current_min(ctypes.byref(w), _ref(b),
                                      int(bound), int(cout), _ptr(out), _stream()))
    v = int(out.item()) & 0xFFFFFFFF
    _current_min_cache.put(key, extra, v)
  return v


def _tb_strides(x, T, B, time_major: bool, unit: int):
  """Element (word) strides of t and b for a contiguous tensor."""
  if time_major:
    return B * unit, unit
  return unit, T * unit


def _zero_step_carry(u_out: Optional[torch.Tensor], u0: Optional[torch.Tensor], T: int):
  """A scan over zero time steps returns its carry (spiking_learning.py:446-462): u0, or the zeros of
  initialize_carry.  The kernels launch nothing for T = 0, so the state is written here."""
  if u_out is not None and T == 0:
    if u0 is None:
      u_out.zero_()
    else:
      u_out.copy_(u0)


def _scan_input(x, time_major: bool, others, weight: Optional[Weight] = None,
                fallback: Optional[FloatFallback] = None, refusal: str = ""):
  """What a fused block reads: (contiguous tensor, in_type, T, B, x_flags).  float32 into the integer
  codes of `weight` needs a FloatFallback (ValueError(refusal) without one) and gets the device word
  x_flags for the kernel to report into; None otherwise."""
  xt, in_type = _in_desc(x)
  xt = xt.contiguous()
  _require_gpu(xt, *others)
  x_flags = None
  if weight is not None and in_type == L.F32 and weight.is_int:
    if fallback is None:
      raise ValueError(refusal)
    x_flags = torch.empty(1, dtype=torch.int32, device=xt.device)
  T, B = (xt.shape[0], xt.shape[1]) if time_major else (xt.shape[1], xt.shape[0])
  return xt, in_type, T, B, x_flags


def _scan_outputs(dev, lead, N: int, u0, want_u: bool, packed_out: bool, state=None, out=None):
  """What a neuron scan writes: (u0 as the kernel reads it, u_T | None, raster tensor, the raster as
  the caller gets it: PackedSpikes iff packed_out).  lead: the raster's leading shape [T, B, ...];
  state: the membrane state's where it is not lead[1:] (the fused pool shrinks the raster only);
  out: the (u_T, raster) of an earlier launch to write again."""
  shape = tuple(lead[1:] if state is None else state) + (N,)
  if out is not None:
    u_out, spikes = out
    s = spikes.bits if isinstance(spikes, PackedSpikes) else spikes
  else:
    u_out = torch.empty(shape, dtype=torch.float32, device=dev) if want_u else None
    s = torch.empty(tuple(lead) + (((N + 31) // 32,) if packed_out else (N,)),
                    dtype=torch.int32 if packed_out else torch.float32, device=dev)
    spikes = PackedSpikes(s, N) if packed_out else s
  if u0 is not None:
    u0 = _f32c(u0)
    assert tuple(u0.shape) == shape, (u0.shape, shape)
  _zero_step_carry(u_out, u0, lead[0])
  return u0, u_out, s, spikes


def conv_lif_forward(x, geom: ConvGeom, weight: Weight, neuron: Neuron,
                     bn: Optional[BnCoeffs] = None, u0: Optional[torch.Tensor] = None,
                     want_u: bool = True, packed_out: bool = False, pool: int = 1,
                     impl: int = L.IMPL_AUTO, time_major: bool = True, x_max: int = 0,
                     x_seen: Optional[torch.Tensor] = None,
                     fallback: Optional[FloatFallback] = None, binary_first: bool = False,
                     logical: Optional[Tuple[int, int, int]] = None):
  """x [T, B, H, W, Cin] (or [B, T, ...] with time_major=False) ->
  (u_T [B, OH, OW, Cout] | None, spikes [T, B, OH/pool, OW/pool, Cout]).
  x_max: the largest input value expected (a hint, snnqp.h); x_seen: eight int32 device words
  that receive the largest uint8 input value the launch met and the chunk counts by maximum.
  fallback: float32 input into integer codes (FloatFallback): the integer launch is followed by
  the predicated float32 one into the same outputs.
  binary_first: uint8 / float32 frames of the 2-channel event layer that are EXPECTED to be binary
  (ops.CountHint.binary_so_far): one checked pass packs them to bits, the event layer runs its
  bit-packed variant on 1/8 (1/32) of the bytes, and a predicated launch on the frames as they are
  redoes the block iff a value was not 0 or 1 (snnqp_pack_frames_checked,
  snnqp_conv_lif_forward_pred) -- same results whatever the frames hold, nothing read back.
  logical: (Cin, Cout, live outputs) of a compacted block, whose launch computes
  geom.Cin x geom.Cout channels: the profile tag keeps the logical geometry, PROFILE_NOTES[tag]
  gets the computed and live counts."""
  xt, in_type, T, B, x_flags = _scan_input(
      x, time_major, (weight.w, u0), weight, fallback,
      "float32 input into integer codes needs a FloatFallback (the float32 kernel)")
  if x_seen is not None:
    assert x_seen.dtype == torch.int32 and x_seen.numel() >= 8 and x_seen.is_cuda, \
        "x_seen: eight int32 device words (snnqp.h)"
  if isinstance(x, PackedFrames):        # [T, B, words / bytes of a frame]
    assert (x.H, x.W, 2) == (geom.H, geom.W, geom.Cin) and xt.ndim == 3, (x.shape, geom)
    unit = xt.shape[-1]
  else:
    unit = geom.H * geom.W * (xt.shape[-1])
  xs_t, xs_b = _tb_strides(xt, T, B, time_major, unit)
  OH, OW = geom.out_hw()
  dev = xt.device
  u0, u_out, s, spikes = _scan_outputs(dev, (T, B, OH // pool, OW // pool), geom.Cout, u0, want_u, packed_out,
                               state=(B, OH, OW))
  g, w, n = geom.struct(), weight.struct(), neuron.struct()
  b = bn.struct() if bn is not None else None
  cin_l, cout_l = (geom.Cin, geom.Cout) if logical is None else logical[:2]
  tag = "conv%dx%d[%dx%dx%d->%d]" % (geom.KH, geom.KW, geom.H, geom.W, cin_l, cout_l)
  if _PROFILE is not None and in_type == L.BITS and weight.is_int and "dequant" not in PROFILE_NOTES.get(tag, {}):
    PROFILE_NOTES.setdefault(tag, {})["dequant"] = conv_dequant_form(weight, neuron)
  if _PROFILE is not None and logical is not None:
    PROFILE_NOTES.setdefault(tag, {})["channels"] = {
        "cin": geom.Cin, "cout": geom.Cout, "live_out": int(logical[2])}
    if weight.cout_fire and packed_out:
      # (the bit-packed launch of binary-first byte frames is the one that can take the half path)
      ev1 = L.EV1 if (in_type == L.EV1 or (binary_first and in_type in (L.U8, L.F32))) else in_type
      PROFILE_NOTES[tag]["channels"]["half_group"] = conv_event_half_group(
          ev1, T, geom, weight, neuron, state=u0 is not None or want_u, pool=pool, x_max=1 if ev1 == L.EV1 else x_max)
      PROFILE_NOTES[tag]["channels"]["wave_spread"] = conv_event_wave_spread(
          ev1, T, geom, weight, neuron, state=u0 is not None or want_u, pool=pool, x_max=1 if ev1 == L.EV1 else x_max)
      PROFILE_NOTES[tag]["channels"]["quarter16"] = conv_event_quarter16(
          ev1, T, geom, weight, neuron, state=u0 is not None or want_u, pool=pool, x_max=1 if ev1 == L.EV1 else x_max)
  # (the bit-packed variant writes bit-packed spikes only: float32 spikes take the frames as they are)
  speculate = (binary_first and packed_out and not isinstance(x, (PackedFrames, PackedSpikes))
               and in_type in (L.U8, L.F32) and geom.Cin == 2 and weight.is_int and impl != L.IMPL_GENERIC
               and xt.ndim == 5)
  with _timed(tag):
    if speculate:
      pf, not_binary = pack_frames_checked(xt)
      ps_t, ps_b = _tb_strides(pf.data, T, B, time_major, pf.data.shape[-1])
      try:
        L.check(L.lib().snnqp_conv_lif_forward(
            _ptr(pf.data), L.EV1, ps_t, ps_b, T, B, ctypes.byref(g), ctypes.byref(w),
            _ptr(weight.wt), _ref(b), ctypes.byref(n),
            _ptr(u0), _ptr(u_out), _ptr(s), L.BITS, pool, impl, 1, None, None, _stream()))
      except L.SnnqpError as e:
        # the bit-packed variant refused the block: nothing has been written to the outputs (only
        # the checked pass has run, into its own buffers) -- the frames go in as they are
        if e.code != L.EUNSUPPORTED:
          raise
        speculate = False
    if speculate:
      # ... and the frames as they are, iff a value was not 0 or 1
      L.check(L.lib().snnqp_conv_lif_forward_pred(
          _ptr(not_binary), _ptr(xt), in_type, xs_t, xs_b, T, B, ctypes.byref(g), ctypes.byref(w),
          _ptr(weight.wt), _ref(b), ctypes.byref(n),
          _ptr(u0), _ptr(u_out), _ptr(s), L.BITS, pool,
          int(x_max), _ptr(x_seen), _ptr(x_flags), _stream()))
    else:
      L.check(L.lib().snnqp_conv_lif_forward(
          _ptr(xt), in_type, xs_t, xs_b, T, B, ctypes.byref(g), ctypes.byref(w),
          _ptr(weight.wt), _ref(b), ctypes.byref(n),
          _ptr(u0), _ptr(u_out), _ptr(s), _out_type(packed_out), pool, impl,
          int(x_max), _ptr(x_seen), _ptr(x_flags), _stream()))
  if fallback is not None:
    # the same block on the float32 kernel, executed only if the word says so (snnqp.h)
    xf = _f32c(xt if fallback.x is None else fallback.x)
    pred = x_flags if fallback.pred is None else fallback.pred
    fw = fallback.weight.struct()
    fs_t, fs_b = _tb_strides(xf, T, B, time_major, geom.H * geom.W * geom.Cin)
    L.check(L.lib().snnqp_conv_lif_forward_if(
        _ptr(pred), _ptr(xf), L.F32, fs_t, fs_b, T, B, ctypes.byref(g), ctypes.byref(fw),
        _ref(b), ctypes.byref(n), _ptr(u0), _ptr(u_out), _ptr(s),
        _out_type(packed_out), pool, _stream()))
  return u_out, spikes


def dense_lif_forward(x, weight: Weight, K: int, N: int, neuron: Neuron,
                      bn: Optional[BnCoeffs] = None, u0: Optional[torch.Tensor] = None,
                      want_u: bool = True, packed_out: bool = False,
                      impl: int = L.IMPL_AUTO, time_major: bool = True,
                      fallback: Optional[FloatFallback] = None):
  """x [T, B, K] -> (u_T [B, N] | None, spikes [T, B, N]).  fallback: as conv_lif_forward."""
  xt, in_type, T, B, x_flags = _scan_input(
      x, time_major, (weight.w, u0), weight, fallback,
      "float32 rows into integer codes need a FloatFallback (the float32 kernel)")
  xs_t, xs_b = _tb_strides(xt, T, B, time_major, xt.shape[-1])
  dev = xt.device
  u0, u_out, s, spikes = _scan_outputs(dev, (T, B), N, u0, want_u, packed_out)
  w, n = weight.struct(), neuron.struct()
  b = bn.struct() if bn is not None else None
  # a long contraction over few rows (the read-out) splits K over workgroups through a workspace
  ws = _dense_workspace(dev, int(L.lib().snnqp_dense_workspace_bytes(in_type, T, B, K, N, ctypes.byref(w)))) \
      if (packed_out and impl != L.IMPL_GENERIC) else None
  with _timed("dense[%d->%d]" % (K, N)):
    L.check(L.lib().snnqp_dense_lif_forward_ws(
        _ptr(xt), in_type, xs_t, xs_b, T, B, K, N, ctypes.byref(w), _ptr(weight.wt),
        _ref(b), ctypes.byref(n), _ptr(u0),
        _ptr(u_out), _ptr(s), _out_type(packed_out), impl, _ptr(x_flags),
        _ptr(ws), 0 if ws is None else ws.numel(), _stream()))
  if fallback is not None:
    xf = _f32c(xt if fallback.x is None else fallback.x)
    pred = x_flags if fallback.pred is None else fallback.pred
    fw = fallback.weight.struct()
    L.check(L.lib().snnqp_dense_lif_forward_if(
        _ptr(pred), _ptr(xf), L.F32, xs_t, xs_b, T, B, K, N, ctypes.byref(fw),
        _ref(b), ctypes.byref(n), _ptr(u0), _ptr(u_out), _ptr(s),
        _out_type(packed_out), _stream()))
  return u_out, spikes


_dense_ws = {}
# workspaces allocated inside the capture that is being recorded: linen.CapturedApply installs a
# list here and keeps it, so that the block is not handed to a later allocation of the same capture
_CAPTURE_KEEP = None


def _dense_workspace(dev, nbytes: int):
  """The workspace of a dense launch that hands partial results over between workgroups
  (snnqp.h: used by one launch at a time; the call zeroes its tickets on the stream), or None.

  Eager launches share one per (device, stream) -- launches of one stream run one after the
  other -- grown as needed.  A launch that is being captured into a hipGraph gets a workspace of
  its OWN, allocated inside the capture, i.e. from the graph's private memory pool: the address
  baked into the graph lives exactly as long as the graph, is never handed to an eager launch and
  never to another graph (two live captures replayed on two streams cannot meet in one).  The
  capture object keeps the tensor (_CAPTURE_KEEP), so no later allocation of the same capture gets
  the block either."""
  if nbytes <= 0:
    return None
  if torch.cuda.is_current_stream_capturing():
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if _CAPTURE_KEEP is not None:
      _CAPTURE_KEEP.append(ws)
    return ws
  key = (torch.device(dev).index, torch.cuda.current_stream(dev).cuda_stream)
  ws = _dense_ws.get(key)
  if ws is None or ws.numel() < nbytes:
    ws = _dense_ws[key] = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
  return ws


def dense_head_forward(x, w1: Weight, K: int, N1: int, nrn1: Neuron, w2: Weight, N2: int,
                       nrn2: Neuron, group: int = 10, want_s1: bool = False,
                       want_s2: bool = False, time_major: bool = True,
                       fallback: Optional[FloatFallback] = None):
  """See _dense_head: the head whose membranes start from zero and are not returned."""
  return _dense_head(x, w1, K, N1, nrn1, w2, N2, nrn2, group, want_s1, want_s2, time_major, fallback, None)[:3]


def dense_head_forward_state(x, w1: Weight, K: int, N1: int, nrn1: Neuron, w2: Weight, N2: int,
                             nrn2: Neuron, u1: torch.Tensor, u2: torch.Tensor, counts: torch.Tensor,
                             group: int = 10, want_s1: bool = False, want_s2: bool = False,
                             time_major: bool = True, fallback: Optional[FloatFallback] = None,
                             workspace: bool = True):
  """The dense head as one launch over one WINDOW of a stream (snnqp_dense_head_forward_state):
  u1 [B, N1], u2 [B, N2] float32 carry the membranes from window to window, counts int32 [B, N2]
  the output spike counts; -> (logits of this window, hidden raster | None, output raster | None,
  u1, u2) where u1 / u2 are the tensors that now hold the state.

  uint8 and bit-packed rows: one launch, which updates u1, u2 and counts in place (each value is
  read and written by the lane that owns it, snnqp.h) and returns the tensors it was given.
  float32 rows are a launch PAIR -- the integer launch, then the predicated float32 redo -- and no
  launch of a window may read a potential another launch of it has written: the integer launch runs
  on copies of u1 / u2 (and counts into a scratch), the redo reads the ORIGINALS and writes the
  copies, and the copies are returned for the caller to keep instead (a swap); counts then take
  the window's output raster, whichever launch wrote it (snnqp_vote_accumulate).
  workspace=False withholds the hand-over workspace: the launch then never splits its columns."""
  for t, n, dt in ((u1, N1, torch.float32), (u2, N2, torch.float32), (counts, N2, torch.int32)):
    if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous() and t.ndim == 2 and t.shape[1] == n):
      raise ValueError("dense_head_forward_state: state tensors are contiguous float32 [B, N1], float32 [B, N2], "
                       "int32 [B, N2]")
  return _dense_head(x, w1, K, N1, nrn1, w2, N2, nrn2, group, want_s1, want_s2, time_major, fallback,
                     (u1, u2, counts), workspace)


def _dense_head(x, w1, K, N1, nrn1, w2, N2, nrn2, group, want_s1, want_s2, time_major, fallback, state,
                workspace=True):
  """The dense head as ONE launch (snnqp_dense_head_forward; examples/tcja/models.py:200-255):
  x [T, B, K] uint8, PackedSpikes or float32 (the rows as the reference holds them, staged in
  place; `fallback` = the float32 kernel of the FIRST block) -> (logits [B, N2 // group], hidden
  raster | None, output raster | None).  Raises SnnqpError(EUNSUPPORTED) when the head does not fit the fused
  kernel; the caller then runs the two blocks and the vote one by one."""
  xt, in_type, T, B, _ = _scan_input(x, time_major, (w1.w, w2.w))   # (its own float32 rule: below)
  xs_t, xs_b = _tb_strides(xt, T, B, time_major, xt.shape[-1])
  dev = xt.device
  if N2 % group:
    raise ValueError("vote: %d features not divisible by group %d" % (N2, group))
  logits = torch.empty((B, N2 // group), dtype=torch.float32, device=dev)
  x_flags = None
  if in_type == L.F32:
    if fallback is None or fallback.x is not None:
      raise ValueError("float32 rows into the fused head need a FloatFallback of the first block")
    x_flags = torch.empty(1, dtype=torch.int32, device=dev)
  elif fallback is not None:
    raise ValueError("a FloatFallback goes with float32 rows; uint8 / bit-packed rows have nothing to redo")
  redo = in_type == L.F32              # the predicated launches go through both rasters
  s1 = torch.empty((T, B, (N1 + 31) // 32), dtype=torch.int32, device=dev) if (want_s1 or redo) else None
  s2 = torch.empty((T, B, (N2 + 31) // 32), dtype=torch.int32, device=dev) if (want_s2 or redo) else None
  a, b, n1, n2 = w1.struct(), w2.struct(), nrn1.struct(), nrn2.struct()
  u1 = u2 = counts = None
  if state is not None:
    u1, u2, counts = state
    _require_gpu(u1, u2, counts)
    if u1.shape[0] != B or u2.shape[0] != B or counts.shape[0] != B:
      raise ValueError("dense_head_forward_state: a state of %d rows for a window of %d" % (u1.shape[0], B))
    if redo:
      u1_0, u2_0, counts_0 = u1, u2, counts
      u1, u2, counts = u1_0.clone(), u2_0.clone(), torch.zeros_like(counts_0)
  # a batch that fills at most half the chip: two workgroups per tile through a workspace
  nws = _head_ws_bytes.get((T, B, N1))
  if nws is None:
    nws = _head_ws_bytes[(T, B, N1)] = int(L.lib().snnqp_dense_head_workspace_bytes(T, B, N1))
  ws = _dense_workspace(dev, nws) if workspace else None
  rasters = (_ptr(s1) if (want_s1 or redo) else None, _ptr(s2) if (want_s2 or redo) else None)
  carried = () if state is None else (_ptr(u1), _ptr(u2), _ptr(counts))
  entry = L.lib().snnqp_dense_head_forward if state is None else L.lib().snnqp_dense_head_forward_state
  with _timed("dense_head%s[%d->%d->%d]" % ("" if state is None else "_state", K, N1, N2)):
    L.check(entry(
        _ptr(xt), in_type, xs_t, xs_b, T, B, K, N1, ctypes.byref(a), _ptr(w1.wt), ctypes.byref(n1),
        N2, ctypes.byref(b), _ptr(w2.wt), ctypes.byref(n2), int(group), *carried, *rasters,
        _ptr(logits), _ptr(x_flags), _ptr(ws), 0 if ws is None else ws.numel(), _stream()))
  if redo:
    # not integer-valued after all: the first block on the float32 kernel, the second (its input
    # is a spike raster whatever produced it) on the integer direct form, the vote -- each
    # executed only if the word says so
    fw = fallback.weight.struct()
    lib = L.lib()
    # (with a carried state: from the potentials the integer launch has NOT touched, into its copies)
    u1_in, u2_in = (None, None) if state is None else (u1_0, u2_0)
    L.check(lib.snnqp_dense_lif_forward_if(_ptr(x_flags), _ptr(xt), L.F32, xs_t, xs_b, T, B, K, N1,
                                           ctypes.byref(fw), None, ctypes.byref(n1), _ptr(u1_in), _ptr(u1), _ptr(s1),
                                           L.BITS, _stream()))
    cw1 = (N1 + 31) // 32
    L.check(lib.snnqp_dense_lif_forward_if(_ptr(x_flags), _ptr(s1), L.BITS, B * cw1, cw1, T, B, N1, N2,
                                           ctypes.byref(b), None, ctypes.byref(n2), _ptr(u2_in), _ptr(u2), _ptr(s2),
                                           L.BITS, _stream()))
    L.check(lib.snnqp_vote_if(_ptr(x_flags), _ptr(s2), L.BITS, T, B, N2, int(group), _ptr(logits), _stream()))
    if state is not None:
      counts = vote_accumulate(PackedSpikes(s2, N2), counts_0)
  return (logits, PackedSpikes(s1, N1) if want_s1 else None,
          PackedSpikes(s2, N2) if want_s2 else None, u1, u2)


_head_ws_bytes = {}


def fallback_counts(reset: bool = False) -> dict:
  """Blocks that IMPL_AUTO handed to the direct-form kernel (20-25 x slower than the MFMA
  kernels) since the library was loaded / the last reset, with the last reason."""
  conv, dense = ctypes.c_int64(), ctypes.c_int64()
  buf = ctypes.create_string_buffer(256)
  L.check(L.lib().snnqp_fallback_counts(ctypes.byref(conv), ctypes.byref(dense), buf, 256,
                                        1 if reset else 0))
  return {"conv_blocks": conv.value, "dense_blocks": dense.value,
          "last_reason": buf.value.decode("utf-8", "replace")}


def device_status(device=None, reset: bool = False) -> int:
  """Codes the kernels of `device` have reported into its status word (_lib.STATUS_*; 0: none) --
  a launch whose bookkeeping did not add up.  While it is not zero the fused block calls raise
  SnnqpError(EHIP); reset=True clears it (after the caller has dealt with the suspect results)."""
  dev = torch.cuda.current_device() if device is None else torch.device(device).index
  code = ctypes.c_uint32()
  L.check(L.lib().snnqp_device_status(int(dev or 0), ctypes.byref(code), 1 if reset else 0))
  return int(code.value)


def workqueue_stats(reset: bool = False) -> dict:
  """Conv launches that walked their patches statically (no capture slot left / eager slot still
  in flight) and bit-input conv launches that ran the arithmetic dequantisation because the
  device did not pass (or, under capture, had not yet run) the denormal probe of the table form."""
  a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
  L.check(L.lib().snnqp_workqueue_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), 1 if reset else 0))
  return {"captured_static_walks": a.value, "busy_static_walks": b.value, "dequant_table_fallbacks": c.value}


def workqueue_capture_mark(device) -> int:
  m = ctypes.c_int64()
  L.check(L.lib().snnqp_workqueue_capture_mark(int(torch.device(device).index or 0), ctypes.byref(m)))
  return int(m.value)


def workqueue_capture_release(device, begin: int, end: int):
  L.check(L.lib().snnqp_workqueue_capture_release(int(torch.device(device).index or 0), int(begin), int(end)))


DQ_FORMS = {1: "arith", 2: "one", 3: "table"}


def conv_event_wave_spread(in_type: int, T: int, geom: ConvGeom, w: Weight, nrn: Neuron, state: bool = False,
                           pool: int = 1, x_max: int = 0) -> bool:
  """Whether snnqp_conv_lif_forward runs this event-layer launch on the spread path
  (snnqp_conv_event_wave_spread): 96 channels on the half-group path or 64 channels off it, the
  bit-packed single-chunk table variant, and nn.set_event_wave_spread is on."""
  gs, ws, ns = geom.struct(), w.struct(), nrn.struct()
  rc = L.lib().snnqp_conv_event_wave_spread(int(in_type), int(T), ctypes.byref(gs), ctypes.byref(ws),
                                            ctypes.byref(ns), 1 if state else 0, int(pool), int(x_max))
  if rc < 0:
    L.check(rc)
  return rc == 1


def conv_event_quarter16(in_type: int, T: int, geom: ConvGeom, w: Weight, nrn: Neuron, state: bool = False,
                         pool: int = 1, x_max: int = 0) -> bool:
  """Whether snnqp_conv_lif_forward runs this event-layer launch with the half group's quarters on the
  16x16x64 matrix instruction (snnqp_conv_event_quarter16): the 96-channel spread launch, and
  nn.set_event_quarter16 is on."""
  gs, ws, ns = geom.struct(), w.struct(), nrn.struct()
  rc = L.lib().snnqp_conv_event_quarter16(int(in_type), int(T), ctypes.byref(gs), ctypes.byref(ws),
                                          ctypes.byref(ns), 1 if state else 0, int(pool), int(x_max))
  if rc < 0:
    L.check(rc)
  return rc == 1


def conv_event_half_group(in_type: int, T: int, geom: ConvGeom, w: Weight, nrn: Neuron, state: bool = False,
                          pool: int = 1, x_max: int = 0) -> bool:
  """Whether snnqp_conv_lif_forward runs this event-layer launch (frame format, T, geometry, weight,
  neuron, membrane state carried in or out, pool, input hint) on the half-group path
  (snnqp_conv_event_half_group): the weight's cout_fire leaves the upper 16 channels of the last
  32-channel group silent, the launch is the bit-packed single-chunk table variant, and
  nn.set_event_half_group is on."""
  gs, ws, ns = geom.struct(), w.struct(), nrn.struct()
  rc = L.lib().snnqp_conv_event_half_group(int(in_type), int(T), ctypes.byref(gs), ctypes.byref(ws),
                                           ctypes.byref(ns), 1 if state else 0, int(pool), int(x_max))
  if rc < 0:
    L.check(rc)
  return rc == 1


def conv_dequant_form(w: Weight, nrn: Neuron) -> str:
  """How the bit-input 3x3 MFMA kernels dequantise with these weights and this neuron
  (snnqp_conv_dequant_form): "arith" (three instructions per value), "one" (L == 1: a
  multiply) or "table" (the accumulator's bit pattern addresses an LDS table)."""
  ws, ns = w.struct(), nrn.struct()
  rc = L.lib().snnqp_conv_dequant_form(ctypes.byref(ws), ctypes.byref(ns))
  if rc < 0:
    L.check(rc)
  return DQ_FORMS[rc]


# ---------------------------------------------------------------------------
# element-wise pieces
# ---------------------------------------------------------------------------


def lif_forward(x: torch.Tensor, neuron: Neuron, bn: Optional[BnCoeffs] = None,
                u0: Optional[torch.Tensor] = None, want_u: bool = True,
                packed_out: bool = False):
  """x float32 [T, ..., C] currents -> (u_T [..., C] | None, spikes [T, ..., C])."""
  x = _f32c(x)
  _require_gpu(x, u0)
  T, C = x.shape[0], x.shape[-1]
  R = (x.numel() // (T * C)) if T * C else 0
  u0, u_out, s, spikes = _scan_outputs(x.device, x.shape[:-1], C, u0, want_u, packed_out)
  n = neuron.struct()
  b = bn.struct() if bn is not None else None
  L.check(L.lib().snnqp_lif_forward(
      _ptr(x), T, R, C, _ref(b), ctypes.byref(n),
      _ptr(u0), _ptr(u_out), _ptr(s), _out_type(packed_out), _stream()))
  return u_out, spikes


def batchnorm_forward(x: torch.Tensor, bn: BnCoeffs) -> torch.Tensor:
  x = _f32c(x)
  _require_gpu(x)
  C = x.shape[-1]
  y = torch.empty_like(x)
  b = bn.struct()
  L.check(L.lib().snnqp_batchnorm_forward(_ptr(x), x.numel() // C if C else 0, C,
                                          ctypes.byref(b), _ptr(y), _stream()))
  return y


def maxpool2x2(x):
  """[..., H, W, C] -> [..., H/2, W/2, C] for float32 tensors or PackedSpikes."""
  t, typ, C = _bits_or_f32(x)
  _require_gpu(t)
  H, W = t.shape[-3], t.shape[-2]
  lead = tuple(t.shape[:-3])
  y = torch.empty(lead + (H // 2, W // 2, t.shape[-1]), dtype=t.dtype, device=t.device)
  L.check(L.lib().snnqp_maxpool2x2(_ptr(t), typ, math.prod(lead), H, W, C, _ptr(y), _stream()))
  return PackedSpikes(y, C) if typ == L.BITS else y


def spatial_mean(x) -> torch.Tensor:
  """[..., H, W, C] (float32 or PackedSpikes) -> float32 [..., C] (mean over H, W)."""
  t, typ, C = _bits_or_f32(x)
  _require_gpu(t)
  lead = tuple(t.shape[:-3])
  HW = t.shape[-3] * t.shape[-2]
  y = torch.empty(lead + (C,), dtype=torch.float32, device=t.device)
  L.check(L.lib().snnqp_spatial_mean(_ptr(t), typ, math.prod(lead), HW, C, _ptr(y), _stream()))
  return y


def sigmoid_gate(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
  a, b = _f32c(a), _f32c(b)
  _require_gpu(a, b)
  assert a.shape == b.shape
  g = torch.empty_like(a)
  L.check(L.lib().snnqp_sigmoid_gate(_ptr(a), _ptr(b), a.numel(), _ptr(g), _stream()))
  return g


def apply_gate(x, g: torch.Tensor) -> torch.Tensor:
  """x [..., H, W, C] * g [..., C] broadcast over H, W -> float32."""
  t, typ, C = _bits_or_f32(x)
  g = _f32c(g)
  _require_gpu(t, g)
  lead = tuple(t.shape[:-3])
  H, W = t.shape[-3], t.shape[-2]
  assert tuple(g.shape) == lead + (C,), (g.shape, lead, C)
  y = torch.empty(lead + (H, W, C), dtype=torch.float32, device=t.device)
  L.check(L.lib().snnqp_apply_gate(_ptr(t), typ, _ptr(g), math.prod(lead), H * W, C, _ptr(y), _stream()))
  return y


def events_to_frames(x, y, p, T: int, H: int, W: int, scale: float = 1.0, as_u8=True):
  """N time-ordered DVS events -> [T, H, W, 2] count frames (input_pipeline.py:142-219)."""
  x = x.to(torch.int32).contiguous()
  y = y.to(torch.int32).contiguous()
  p = p.to(torch.int32).contiguous()
  _require_gpu(x, y, p)
  counts = torch.empty((T, H, W, 2), dtype=torch.int32, device=x.device)
  u8 = torch.empty((T, H, W, 2), dtype=torch.uint8, device=x.device) if as_u8 else None
  L.check(L.lib().snnqp_events_to_frames(_ptr(x), _ptr(y), _ptr(p), x.numel(), T, H, W,
                                         float(scale), _ptr(counts), _ptr(u8), _stream()))
  return u8 if as_u8 else counts


EVENT_COORD_MAX = (1 << 14) - 1
EVENT_MODES = {"number": 0, "time": 1}


def _host_array(a, name):
  import numpy as np
  if isinstance(a, torch.Tensor):
    a = a.detach().cpu().numpy()
  a = np.asarray(a)
  if a.size == 0:
    a = a.astype(np.int64)
  if a.dtype.kind not in "iu":
    raise ValueError("%s must be integers, got %s" % (name, a.dtype))
  return a


class EventSet:
  """The raw DVS events of a split, resident on `device` for `events_bin`: S ragged samples back to
  back, sample s owning events offsets[s] .. offsets[s + 1] - 1.

  addrs [N, 3] integer (x, y, polarity) rows are packed into one word per event (x in bits 0..13,
  y in bits 14..27, polarity != 0 in bit 28; a coordinate outside 0..16383 is refused), `times`
  are cast to int32 as the reference casts them (examples/input_pipeline.py:72; a value that
  does not fit is refused), `offsets` must start at 0, never decrease and end at N.  A sample
  whose times decrease somewhere is sorted stably by time, once, and `sorted_by_time` remembers
  it: counts in time mode do not depend on the order inside a window, but in number mode the
  order IS the result, so such a set refuses number mode.  t_min / t_max (numpy int64 [S], 0 for
  an empty sample) stay on the host: the window origins are drawn there."""

  def __init__(self, addrs, times, offsets, sensor_size, device=None):
    import numpy as np
    if device is None:
      device = addrs.device if isinstance(addrs, torch.Tensor) else torch.device("cpu")
    a = _host_array(addrs, "addrs")
    t = _host_array(times, "times").reshape(-1)
    off = _host_array(offsets, "offsets").reshape(-1).astype(np.int64)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] != t.shape[0]:
      raise ValueError("addrs must be [N, 3] (x, y, polarity) with one time per event, got %s / %s"
                       % (a.shape, t.shape))
    n = a.shape[0]
    if off.shape[0] < 1 or off[0] != 0 or off[-1] != n or np.any(np.diff(off) < 0):
      raise ValueError("offsets must start at 0, never decrease and end at the event count %d" % n)
    if n and (int(a[:, :2].min()) < 0 or int(a[:, :2].max()) > EVENT_COORD_MAX):
      raise ValueError("event coordinates must lie in 0..%d, got %d..%d"
                       % (EVENT_COORD_MAX, int(a[:, :2].min()), int(a[:, :2].max())))
    if n and (int(t.min()) < -2 ** 31 or int(t.max()) > 2 ** 31 - 1):
      raise ValueError("event times %d..%d do not fit int32 microseconds" % (int(t.min()), int(t.max())))
    t = t.astype(np.int32)
    word = (a[:, 0].astype(np.int64) | (a[:, 1].astype(np.int64) << 14)
            | ((a[:, 2] != 0).astype(np.int64) << 28)).astype(np.int32)
    S = off.shape[0] - 1
    self.sorted_by_time = False
    if n > 1:
      down = np.flatnonzero(np.diff(t.astype(np.int64)) < 0) + 1       # event i is earlier than event i - 1
      down = down[~np.isin(down, off)]                                 # (a sample's first event may be)
      for s in np.unique(np.searchsorted(off, down, side="right") - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        order = np.argsort(t[lo:hi], kind="stable")
        t[lo:hi], word[lo:hi] = t[lo:hi][order], word[lo:hi][order]
        self.sorted_by_time = True
    self.t_min, self.t_max = np.zeros(S, np.int64), np.zeros(S, np.int64)
    full = np.flatnonzero(off[1:] > off[:-1])
    self.t_min[full] = t[off[:-1][full]]
    self.t_max[full] = t[off[1:][full] - 1]
    hw = np.asarray(sensor_size).reshape(-1)
    self.sensor_size = (int(hw[0]), int(hw[-1]))                       # (H, W); one number: square
    self.num_samples, self.num_events = S, n
    self.counts = np.diff(off)
    self.addr = torch.from_numpy(word).to(device)
    self.times = torch.from_numpy(t).to(device)
    # what the launch is handed: a set without a single event still has an array to point at
    self._addr_arg = self.addr if n else torch.zeros(1, dtype=torch.int32, device=device)
    self._times_arg = self.times if n else torch.zeros(1, dtype=torch.int32, device=device)
    self.offsets = torch.from_numpy(off).to(device)

  @property
  def device(self):
    return self.addr.device

  def unpack(self) -> torch.Tensor:
    """The events as int32 [N, 3] (x, y, polarity 0 / 1) rows, on the device of the set."""
    w = self.addr
    return torch.stack([w & EVENT_COORD_MAX, (w >> 14) & EVENT_COORD_MAX, (w >> 28) & 1], 1)

  def __repr__(self):
    return "EventSet(%d samples, %d events, sensor %s, device=%s)" % (
        self.num_samples, self.num_events, self.sensor_size, self.device)


def _event_rows(v, name, B=None, lo=-2 ** 31, hi=2 ** 31 - 1):
  """int32 host tensor of a per-row argument of events_bin, validated before upload."""
  import numpy as np
  a = _host_array(v, name).reshape(-1).astype(np.int64)
  if B is not None and a.shape[0] != B:
    raise ValueError("%s must have one entry per batch row (%d), got %d" % (name, B, a.shape[0]))
  if a.size and (int(a.min()) < lo or int(a.max()) > hi):
    raise ValueError("%s must lie in %d..%d, got %d..%d" % (name, lo, hi, int(a.min()), int(a.max())))
  return torch.from_numpy(a.astype(np.int32))


EVENT_SHIFT_MAX = 1 << 14


class EventAugment:
  """Per-row event augmentation of one `events_bin` batch of `rows` rows (snnqp_event_aug_t,
  include/snnqp.h, which states the order the rules apply in).  Every argument is a host array with
  one entry per row; an absent one is the identity:

    flip_x, flip_y, swap_polarity   booleans
    dx, dy          the shift in frame pixels, |.| <= 16384; what leaves the frame is dropped
    cutout          [rows, 4] (x0, y0, x1, y1), half-open, in final frame pixels, int32; empty when
                    x1 <= x0 or y1 <= y0
    frames          [rows, 2] (f0, f1): frames [f0, f1) come out empty, 0 <= f0 <= f1 (<= T is
                    checked where T is known, in `records`)
    drop_below      event i of the row's sample is dropped when its hash under `seed` is below
                    this: a drop probability p is floor(p * 2^32); both in 0 .. 2^32 - 1

  Everything is validated here, on the host; the arrays are kept as int64 attributes of the same
  names."""

  def __init__(self, rows: int, *, flip_x=None, flip_y=None, swap_polarity=None, dx=None, dy=None,
               cutout=None, frames=None, drop_below=None, seed=None):
    import numpy as np
    self.rows = B = int(rows)
    if B < 0:
      raise ValueError("rows must be >= 0, got %d" % B)

    def field(v, name, lo, hi, width=None):
      shape = (B,) if width is None else (B, width)
      if v is None:
        return np.zeros(shape, np.int64)
      a = _host_array(v, name)
      if a.dtype == np.uint64 and a.size and int(a.max()) > hi:
        raise ValueError("%s must lie in %d..%d, got up to %d" % (name, lo, hi, int(a.max())))
      a = a.astype(np.int64)
      if a.shape != shape:
        raise ValueError("%s must have shape %s, one entry per batch row, got %s" % (name, shape, a.shape))
      if a.size and (int(a.min()) < lo or int(a.max()) > hi):
        raise ValueError("%s must lie in %d..%d, got %d..%d" % (name, lo, hi, int(a.min()), int(a.max())))
      return a

    def flag(v, name):
      if v is not None and not isinstance(v, torch.Tensor):
        v = np.asarray(v)
        v = v.astype(np.int64) if v.dtype == np.bool_ else v
      elif v is not None:
        v = v.to(torch.int64)
      return field(v, name, 0, 1)

    self.flip_x, self.flip_y = flag(flip_x, "flip_x"), flag(flip_y, "flip_y")
    self.swap_polarity = flag(swap_polarity, "swap_polarity")
    self.dx = field(dx, "dx", -EVENT_SHIFT_MAX, EVENT_SHIFT_MAX)
    self.dy = field(dy, "dy", -EVENT_SHIFT_MAX, EVENT_SHIFT_MAX)
    self.cutout = field(cutout, "cutout", -2 ** 31, 2 ** 31 - 1, 4)
    self.frames = field(frames, "frames", 0, 2 ** 31 - 1, 2)
    if np.any(self.frames[:, 0] > self.frames[:, 1]):
      raise ValueError("frames must be (f0, f1) with 0 <= f0 <= f1, got %s" % self.frames.tolist())
    self.drop_below = field(drop_below, "drop_below", 0, 2 ** 32 - 1)
    self.seed = field(seed, "seed", 0, 2 ** 32 - 1)

  def records(self, T: int):
    """The rows as snnqp_event_aug_t records: numpy int32 [rows, 12] (the unsigned fields as their
    bit patterns).  Refuses a frame range that ends beyond T."""
    import numpy as np
    if self.rows and int(self.frames[:, 1].max()) > int(T):
      raise ValueError("frames must end at or before T = %d, got f1 up to %d" % (T, int(self.frames[:, 1].max())))
    r = np.zeros((self.rows, 12), np.int64)
    r[:, 0] = self.flip_x | (self.flip_y << 1) | (self.swap_polarity << 2)
    r[:, 1], r[:, 2] = self.dx, self.dy
    r[:, 3:7] = self.cutout
    r[:, 7:9] = self.frames
    r[:, 9], r[:, 10] = self.drop_below, self.seed
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.int32)

  def __repr__(self):
    return "EventAugment(%d rows)" % self.rows


class EventMix:
  """Per-row mixing of one `events_bin` batch of `rows` rows with a partner sample each
  (snnqp_events_bin_mix, include/snnqp.h): inside the row's box the partner's events
  are counted, outside it the row's own.  Host arrays with one entry per row:

    partner   the partner sample, in [0, S) (checked where S is known, in `events_bin`), or -1 for
              a row that is not mixed
    start     the partner's window origin, int32; time mode only (None in number mode)
    box       [rows, 6] (x0, y0, x1, y1, g0, g1), int32: final frame pixels and frames, half-open,
              0 <= g0 <= g1 (<= T is checked where T is known, in `records`); empty when
              x1 <= x0, y1 <= y0 or g1 <= g0
    augment   the partner rows' EventAugment (their flips, shifts, drops ...), or None

  Everything is validated here, on the host; the arrays are kept as int64 attributes."""

  def __init__(self, rows: int, *, partner, start=None, box, augment: Optional[EventAugment] = None):
    import numpy as np
    self.rows = B = int(rows)
    if B < 0:
      raise ValueError("rows must be >= 0, got %d" % B)
    self.partner = _event_rows(partner, "partner", B, lo=-1).numpy().astype(np.int64)
    self.start = None if start is None else _event_rows(start, "mix start", B).numpy().astype(np.int64)
    a = _host_array(box, "box")
    if a.shape != (B, 6):
      raise ValueError("box must have shape %s, (x0, y0, x1, y1, g0, g1) per batch row, got %s" % ((B, 6), a.shape))
    if a.dtype == np.uint64 and a.size and int(a.max()) > 2 ** 31 - 1:
      raise ValueError("box must lie in %d..%d, got up to %d" % (-2 ** 31, 2 ** 31 - 1, int(a.max())))
    a = a.astype(np.int64)
    if a.size and (int(a.min()) < -2 ** 31 or int(a.max()) > 2 ** 31 - 1):
      raise ValueError("box must lie in %d..%d, got %d..%d" % (-2 ** 31, 2 ** 31 - 1, int(a.min()), int(a.max())))
    if np.any(a[:, 4] < 0) or np.any(a[:, 4] > a[:, 5]):
      raise ValueError("box frames must be (g0, g1) with 0 <= g0 <= g1, got %s" % a[:, 4:].tolist())
    self.box = a
    if augment is not None:
      if not isinstance(augment, EventAugment):
        raise ValueError("a mix's augment must be an ops.EventAugment, got %r" % (type(augment).__name__,))
      if augment.rows != B:
        raise ValueError("a mix's augment must have one record per batch row (%d), got %d" % (B, augment.rows))
    self.augment = augment

  def records(self, T: int):
    """(partner int32 [rows], box int32 [rows, 6], the partners' aug records int32 [rows, 12] or
    None) as the launch reads them.  Refuses a box or a frame range that ends beyond T."""
    import numpy as np
    if self.rows and int(self.box[:, 5].max()) > int(T):
      raise ValueError("box frames must end at or before T = %d, got g1 up to %d" % (T, int(self.box[:, 5].max())))
    return (self.partner.astype(np.int32), self.box.astype(np.int32),
            None if self.augment is None else self.augment.records(T))

  def __repr__(self):
    return "EventMix(%d rows, %d mixed)" % (self.rows, int((self.partner >= 0).sum()))


def events_bin(events: EventSet, sample, T: int, H: int, W: int, *, mode, start=None, step_us=None,
               scale: float = 1.0, fmt: Optional[int] = None, flags: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, augment: Optional[EventAugment] = None,
               mix: Optional[EventMix] = None):
  """One launch (snnqp_events_bin): row b of the batch decodes sample[b] of `events` into T frames of
  H x W x 2 counts.  mode "number": equal-count slices (input_pipeline.py:142-219); mode "time":
  windows of step_us microseconds from start[b], both edges strict (:63-131).  Returns uint8
  [B, T, H, W, 2] (saturated at 255), or PackedFrames for fmt _lib.EV4 / _lib.EV1, saturated at
  15 / 1 with FLAG_GT_15 / FLAG_GT_ONE OR-ed into the int32 device word `flags` when one is
  given.  `sample` (each in [0, S)) and `start` (int32) are validated here, on the host.  `out`,
  when given, is the tensor the launch writes -- uint8 [B, T, H, W, 2] or the packed data
  [B, T, units] --, every element of it.  `augment`, an EventAugment of B rows, makes it the
  augmenting launch (snnqp_events_bin_aug): flips, shift, cutout, hashed drops, polarity swap and
  emptied frames per row, its records in the same upload as `sample` and `start`; None is the
  plain launch.  `mix`, an EventMix of B rows, makes it the mixing launch (snnqp_events_bin_mix):
  inside each mixed row's box the partner sample's events are counted, under the mix's own augment;
  everything still goes up in that one upload, and the call returns (frames, counts) with counts
  an int64 [B, 2] device tensor -- the row's own and its partner's events that were counted --,
  which nothing here reads back."""
  m = EVENT_MODES.get(mode, mode)
  if m not in (0, 1):
    raise ValueError("mode must be 'number' or 'time', got %r" % (mode,))
  if fmt not in (None, L.U8, L.EV1, L.EV4):
    raise ValueError("fmt must be None (uint8), _lib.EV1 or _lib.EV4, got %r" % (fmt,))
  if m == 0 and events.sorted_by_time:
    raise ValueError("this EventSet had to sort a sample by time: number mode, whose result is the "
                     "order of the events, is refused")
  T, H, W = int(T), int(H), int(W)
  rows = _event_rows(sample, "sample", lo=0, hi=events.num_samples - 1)
  B = rows.shape[0]
  if m == 1:
    if start is None or step_us is None:
      raise ValueError("time mode needs start and step_us")
    starts = _event_rows(start, "start", B)
    if int(step_us) <= 0 or int(step_us) > 2 ** 31 - 1:
      raise ValueError("step_us must be a positive int32, got %r" % (step_us,))
  else:
    starts = None
  if augment is not None:
    if not isinstance(augment, EventAugment):
      raise ValueError("augment must be an ops.EventAugment, got %r" % (type(augment).__name__,))
    if augment.rows != B:
      raise ValueError("augment must have one record per batch row (%d), got %d" % (B, augment.rows))
    records = augment.records(T)
  if mix is not None:
    import numpy as np
    if not isinstance(mix, EventMix):
      raise ValueError("mix must be an ops.EventMix, got %r" % (type(mix).__name__,))
    if mix.rows != B:
      raise ValueError("mix must have one entry per batch row (%d), got %d" % (B, mix.rows))
    if B and int(mix.partner.max()) >= events.num_samples:
      raise ValueError("mix partner must lie in -1..%d, got up to %d" % (events.num_samples - 1, int(mix.partner.max())))
    if m == 1 and mix.start is None:
      raise ValueError("time mode needs the mix's start: the partners' window origins")
    partner, box, records2 = mix.records(T)
  _require_gpu(events.addr, flags, out)
  dev = events.device
  packed = fmt in (L.EV1, L.EV4)
  shape = (B, T, frame_units(H, W, fmt)) if packed else (B, T, H, W, 2)
  dtype = torch.int32 if fmt == L.EV1 else torch.uint8
  if out is None:
    out = torch.empty(shape, dtype=dtype, device=dev)
  elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous():
    raise ValueError("out must be a contiguous %s tensor of shape %s" % (dtype, shape))
  if mix is not None:
    counts = torch.zeros((B, 2), dtype=torch.int64, device=dev)
    if B and T:
      parts, at, n = [], {}, 0
      for name, part in (("rows", rows), ("start", starts), ("aug", None if augment is None else records),
                         ("partner", partner), ("start2", mix.start if m == 1 else None), ("box", box), ("aug2", records2)):
        if part is not None:
          if not isinstance(part, torch.Tensor):
            part = torch.from_numpy(np.ascontiguousarray(part, dtype=np.int32))
          parts.append(part.reshape(-1))
          at[name] = (n, n + part.numel())
          n += part.numel()
      both = torch.cat(parts).to(dev)                                              # one upload
      arg = lambda name: _ptr(both[at[name][0]:at[name][1]]) if name in at else None
      L.check(L.lib().snnqp_events_bin_mix(_ptr(events._addr_arg), _ptr(events._times_arg), _ptr(events.offsets),
                                           events.num_samples, arg("rows"), arg("start"), arg("aug"), arg("partner"),
                                           arg("start2"), arg("aug2"), arg("box"), _ptr(counts), B, m, T,
                                           int(step_us) if m == 1 else 0, H, W, float(scale), _ptr(out),
                                           fmt if packed else L.U8, _ptr(flags), _stream()))
    return (PackedFrames(out, H, W, fmt) if packed else out), counts
  if B and T and augment is not None:
    host = torch.cat([rows] + ([] if starts is None else [starts]) + [torch.from_numpy(records).reshape(-1)])
    both = host.to(dev)                                                          # one upload
    rows_d, starts_d = both[:B], (None if starts is None else both[B:2 * B])
    L.check(L.lib().snnqp_events_bin_aug(_ptr(events._addr_arg), _ptr(events._times_arg), _ptr(events.offsets),
                                         events.num_samples, _ptr(rows_d), _ptr(starts_d), B, m, T,
                                         int(step_us) if m == 1 else 0, H, W, float(scale),
                                         _ptr(both[both.shape[0] - 12 * B:]), _ptr(out),
                                         fmt if packed else L.U8, _ptr(flags), _stream()))
  elif B and T:
    both = (rows if starts is None else torch.stack([rows, starts])).to(dev)     # one upload
    rows_d, starts_d = (both, None) if starts is None else (both[0], both[1])
    L.check(L.lib().snnqp_events_bin(_ptr(events._addr_arg), _ptr(events._times_arg), _ptr(events.offsets),
                                     events.num_samples, _ptr(rows_d), _ptr(starts_d), B, m, T,
                                     int(step_us) if m == 1 else 0, H, W, float(scale), _ptr(out),
                                     fmt if packed else L.U8, _ptr(flags), _stream()))
  return PackedFrames(out, H, W, fmt) if packed else out


class ImageSet:
  """The static images of a split, resident on `device` for `rate_encode`: uint8 [N, ...] (a numpy
  array or a tensor), kept as [N, K] with K the product of the other axes; `item_shape` remembers
  them.  Anything but uint8 is refused; N = 0 is allowed."""

  def __init__(self, images, device=None):
    import numpy as np
    if isinstance(images, torch.Tensor):
      if device is None:
        device = images.device
      x = images.detach()
    else:
      x = np.asarray(images)
      if x.dtype != np.uint8:
        raise ValueError("images must be uint8, got %s" % (x.dtype,))
      x = torch.from_numpy(np.ascontiguousarray(x))
      if device is None:
        device = torch.device("cpu")
    if x.dtype != torch.uint8:
      raise ValueError("images must be uint8, got %s" % (x.dtype,))
    if x.ndim < 1:
      raise ValueError("images must be [N, ...], got a scalar")
    self.item_shape = tuple(int(d) for d in x.shape[1:])
    self.num_samples = int(x.shape[0])
    self.K = int(math.prod(self.item_shape))
    self.data = x.reshape(self.num_samples, self.K).contiguous().to(device)

  @property
  def device(self):
    return self.data.device

  def __repr__(self):
    return "ImageSet(%d images of %s, device=%s)" % (self.num_samples, self.item_shape, self.device)


ENCODE_KINDS = {"bernoulli": L.ENCODE_BERNOULLI, "poisson": L.ENCODE_POISSON}
ENCODE_COUNT_MAX = 15


class RateTable:
  """The 256 x 16 thresholds `rate_encode` compares its hashes with (include/snnqp.h), built on the
  host in float64.  A pixel value v has the rate r(v) = max(0, gain * ((v / 255 - mean) / std)): a
  negative rate encodes as 0.
    bernoulli  entry 0 = min(floor(min(r, 1) * 2^32), 2^32 - 1): a spike iff the hash is below it
               (2^32 - 1 stands for 2^32, always); the other entries are 0
    poisson    entry j < 15 = min(floor(P(X <= j; r) * 2^32), 2^32 - 1), P accumulated in ascending j
               from exp(-r), each term the previous one times r / j; the count is the number of
               entries the hash is at or above, so it saturates at 15; entry 15 is 0
  `entries` is the numpy uint32 [256, 16] table, `rates` the float64 [256] rates, and
  `truncated_mass` the largest P(X > 15) over the 256 values: what the cap at 15 costs (0.0 for
  bernoulli).  `on(device)` is the table on a device, uploaded once per device."""

  def __init__(self, kind, gain: float = 1.0, mean: float = 0.0, std: float = 1.0):
    import numpy as np
    if kind not in ENCODE_KINDS:
      raise ValueError("kind must be one of %s, got %r" % (sorted(ENCODE_KINDS), kind))
    gain, mean, std = float(gain), float(mean), float(std)
    if not (math.isfinite(gain) and math.isfinite(mean) and math.isfinite(std)):
      raise ValueError("gain, mean and std must be finite, got %r, %r, %r" % (gain, mean, std))
    if std <= 0.0:
      raise ValueError("std must be positive, got %r" % (std,))
    self.kind, self.gain, self.mean, self.std = kind, gain, mean, std
    self.code = ENCODE_KINDS[kind]
    r = np.maximum(0.0, gain * ((np.arange(256, dtype=np.float64) / 255.0 - mean) / std))
    top = 2.0 ** 32
    e = np.zeros((256, 16), np.float64)
    self.truncated_mass = 0.0
    if kind == "bernoulli":
      e[:, 0] = np.floor(np.minimum(r, 1.0) * top)
    else:
      term = np.exp(-r)
      cdf = term.copy()
      e[:, 0] = np.floor(cdf * top)
      for j in range(1, ENCODE_COUNT_MAX + 1):
        term = term * (r / j)
        cdf = cdf + term
        if j < ENCODE_COUNT_MAX:
          e[:, j] = np.floor(cdf * top)
      self.truncated_mass = float(np.max(np.clip(1.0 - cdf, 0.0, 1.0)))      # cdf: P(X <= 15)
    self.rates = r
    self.entries = np.minimum(e, top - 1.0).astype(np.uint32)
    self._on = {}

  def on(self, device) -> torch.Tensor:
    """The table as an int32 [256, 16] tensor (the uint32 bit patterns) on `device`."""
    import numpy as np
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
      device = torch.device("cuda", torch.cuda.current_device())
    t = self._on.get(device)
    if t is None:
      t = self._on[device] = torch.from_numpy(self.entries.view(np.int32).copy()).to(device)
    return t

  def __repr__(self):
    return "RateTable(%r, gain=%r, mean=%r, std=%r)" % (self.kind, self.gain, self.mean, self.std)


def rate_encode(images: ImageSet, sample, T: int, table: RateTable, *, seed, draw=0, sample_id=None,
                fmt: str = "u8", time_major: bool = False):
  """One launch (snnqp_rate_encode): row b of the batch encodes image sample[b] of `images` into T
  steps of K rate-coded elements under `table`.  Returns uint8 [B, T, K] (0 / 1 for a bernoulli
  table, counts 0..15 for a poisson one) or, fmt "bits" (bernoulli only), PackedSpikes of that
  shape; time_major=True gives [T, B, K].  `sample` is a host integer array, each entry in [0, N),
  validated here; `sample_id` (default: `sample`) are the ids that go into the hash -- the samples'
  indices in the whole source when `images` is one rank's slice --, taken modulo 2^32 as `seed`
  and `draw` are.  The value at (sample_id, t, k) depends on seed, draw and the pixel alone."""
  import numpy as np
  if not isinstance(images, ImageSet):
    raise ValueError("images must be an ops.ImageSet, got %r" % (type(images).__name__,))
  if not isinstance(table, RateTable):
    raise ValueError("table must be an ops.RateTable, got %r" % (type(table).__name__,))
  if fmt not in ("u8", "bits"):
    raise ValueError("fmt must be 'u8' or 'bits', got %r" % (fmt,))
  if fmt == "bits" and table.kind != "bernoulli":
    raise ValueError("fmt 'bits' holds spikes: it needs a bernoulli table, got %r" % (table.kind,))
  T, K = int(T), images.K
  if T < 0:
    raise ValueError("T must be >= 0, got %d" % T)
  if K < 1 or T * K >= 2 ** 32:
    raise ValueError("rate_encode needs K >= 1 and T * K < 2^32, got T = %d, K = %d" % (T, K))
  rows = _event_rows(sample, "sample", lo=0, hi=images.num_samples - 1)
  B = rows.shape[0]
  if sample_id is None:
    ids = rows
  else:
    ids = _host_array(sample_id, "sample_id").reshape(-1)
    if ids.shape[0] != B:
      raise ValueError("sample_id must have one entry per batch row (%d), got %d" % (B, ids.shape[0]))
    ids = np.array([int(i) % 2 ** 32 for i in ids.tolist()], np.int64)          # (uint64 ids too)
    ids = torch.from_numpy(ids.astype(np.uint32).view(np.int32))
  _require_gpu(images.data)
  dev = images.device
  unit = (K + 31) // 32 if fmt == "bits" else K
  shape = (T, B, unit) if time_major else (B, T, unit)
  out = torch.empty(shape, dtype=torch.int32 if fmt == "bits" else torch.uint8, device=dev)
  if B and T:
    os_t, os_b = _tb_strides(out, T, B, time_major, unit)
    both = torch.stack([rows, ids]).to(dev)                                        # one upload
    L.check(L.lib().snnqp_rate_encode(_ptr(images.data), images.num_samples, _ptr(both[0]), _ptr(both[1]), B, T, K,
                                      int(seed) % 2 ** 32, int(draw) % 2 ** 32, _ptr(table.on(dev)), table.code,
                                      _ptr(out), L.BITS if fmt == "bits" else L.U8, os_b, os_t, _stream()))
  return PackedSpikes(out, K) if fmt == "bits" else out


def density(x, lead_dims: int = 2, counts: bool = False) -> torch.Tensor:
  """Fraction of non-zero activations of each leading slice (default per [T, B]),
  the probe of examples/tcja/models.py:128-142; float32 of shape x.shape[:lead_dims]
  (or the exact int32 non-zero counts with counts=True)."""
  if isinstance(x, PackedFrames):
    x = unpack_frames(x)
  if isinstance(x, GatedSpikes):
    x = x.to_dense()
  if isinstance(x, PackedSpikes):
    t, typ, C, shape = x.bits, L.BITS, x.channels, x.shape
  elif x.dtype == torch.uint8:
    t, typ, C, shape = x.contiguous(), L.U8, x.shape[-1], tuple(x.shape)
  else:
    t, typ, C, shape = _f32c(x), L.F32, x.shape[-1], tuple(x.shape)
  _require_gpu(t)
  lead = tuple(shape[:lead_dims])
  NB = math.prod(lead)
  n = 1
  for d in shape[lead_dims:]:
    n *= d
  nnz = torch.empty(lead, dtype=torch.int32, device=t.device)
  L.check(L.lib().snnqp_density(_ptr(t), typ, NB, n, C, _ptr(nnz), _stream()))
  if counts:
    return nnz
  return nnz.to(torch.float32) / float(n)


def vote(s, group: int = 10) -> torch.Tensor:
  """spikes [T, B, N] -> logits float32 [B, N // group] (models.py:253-255)."""
  t, typ, N = _bits_or_f32(s)
  _require_gpu(t)
  T, B = t.shape[0], t.shape[1]
  if N % group:
    raise ValueError("vote: %d features not divisible by group %d" % (N, group))
  out = torch.empty((B, N // group), dtype=torch.float32, device=t.device)
  L.check(L.lib().snnqp_vote(_ptr(t), typ, T, B, N, group, _ptr(out), _stream()))
  return out


def vote_accumulate(s, counts: torch.Tensor) -> torch.Tensor:
  """spikes [T, B, N] of one window: each neuron's spike count is added into counts int32 [B, N],
  in place (snnqp_vote_accumulate); returns counts."""
  t, typ, N = _bits_or_f32(s)
  _require_gpu(t, counts)
  T, B = t.shape[0], t.shape[1]
  if not (counts.dtype == torch.int32 and counts.is_contiguous() and tuple(counts.shape) == (B, N)):
    raise ValueError("vote_accumulate: counts must be contiguous int32 [%d, %d], got %s %s"
                     % (B, N, counts.dtype, tuple(counts.shape)))
  L.check(L.lib().snnqp_vote_accumulate(_ptr(t), typ, T, B, N, _ptr(counts), _stream()))
  return counts


def vote_counts(counts: torch.Tensor, steps, group: int = 10) -> torch.Tensor:
  """counts int32 [B, N] over `steps` time steps -> logits float32 [B, N // group], the bits ops.vote
  gives for the raster the counts were taken from (snnqp_vote_counts).  steps: an int, or an int32
  device tensor [B] with every row's own number of steps (a row with none votes 0)."""
  _require_gpu(counts)
  B, N = counts.shape
  if N % group:
    raise ValueError("vote: %d features not divisible by group %d" % (N, group))
  if not (counts.dtype == torch.int32 and counts.is_contiguous()):
    raise ValueError("vote_counts: counts must be contiguous int32")
  per_row = isinstance(steps, torch.Tensor)
  if per_row:
    _require_gpu(steps)
    if not (steps.dtype == torch.int32 and steps.is_contiguous() and tuple(steps.shape) == (B,)):
      raise ValueError("vote_counts: per-row steps must be contiguous int32 [%d]" % B)
  out = torch.empty((B, N // group), dtype=torch.float32, device=counts.device)
  L.check(L.lib().snnqp_vote_counts(_ptr(counts), 0 if per_row else int(steps), _ptr(steps) if per_row else None,
                                    B, N, group, _ptr(out), _stream()))
  return out


# ---------------------------------------------------------------------------
# training of the dense blocks (csrc/train_dense.hip)
# ---------------------------------------------------------------------------


def _window_state(who, name, u, shape, device):
  """A window's membrane-shaped operand (u0, gu_T): float32, contiguous, [R, C] in any leading
  shape; None stays None (the kernels read zeros)."""
  if u is None:
    return None
  if not isinstance(u, torch.Tensor) or u.numel() != math.prod(shape):
    raise ValueError("%s: %s must hold the %d membranes of one step %s, got %s"
                     % (who, name, math.prod(shape), tuple(shape),
                        tuple(u.shape) if isinstance(u, torch.Tensor) else type(u).__name__))
  u = _f32c(u)
  _require_gpu(u)
  return u


def _forward_save(who, entry, entry_state, x, neuron, u0, return_state):
  x = _f32c(x)
  _require_gpu(x)
  T, C = x.shape[0], x.shape[-1]
  step = tuple(x.shape[1:])
  R = (math.prod(step) // C) if C else 0
  h = torch.empty_like(x)
  s = torch.empty_like(x)
  if u0 is None and not return_state:
    L.check(entry(_ptr(x), T, R if T else 0, C, ctypes.byref(neuron.struct()), _ptr(h), _ptr(s), _stream()))
    return h, s
  u0 = _window_state(who, "u0", u0, step, x.device)
  u_out = torch.empty(step, dtype=torch.float32, device=x.device) if return_state else None
  L.check(entry_state(_ptr(x), T, R, C, ctypes.byref(neuron.struct()), _ptr(u0), _ptr(u_out),
                      _ptr(h), _ptr(s), _stream()))
  return (h, s, u_out) if return_state else (h, s)


def lif_forward_save(x: torch.Tensor, neuron: Neuron, u0: Optional[torch.Tensor] = None,
                     return_state: bool = False):
  """currents float32 [T, ..., C] -> (h, s) float32 [T, ..., C]: the multi_step_LIF potential
  before the reset and the spikes, from a zero state (the arithmetic of lif_forward).

  u0 float32 [..., C]: the membrane the scan starts from (a window of a recording);
  return_state: -> (h, s, u_T) with u_T [..., C] the membrane after the last step (u0 itself for
  T == 0).  With neither, the call is the one it was (snnqp_lif_forward_save)."""
  lib = L.lib()
  return _forward_save("lif_forward_save", lib.snnqp_lif_forward_save, lib.snnqp_lif_forward_save_state,
                       x, neuron, u0, return_state)


def lif_backward(h: torch.Tensor, neuron: Neuron, surrogate: int, gs: Optional[torch.Tensor] = None,
                 glogits: Optional[torch.Tensor] = None, group: int = 10,
                 u0: Optional[torch.Tensor] = None, gu_T: Optional[torch.Tensor] = None,
                 return_gu0: bool = False):
  """BPTT of the multi_step_LIF scan: h [T, R, C] -> gI [T, R, C], from the spikes' gradient
  gs [T, R, C] or, through the vote, from the logits' gradient glogits [R, C // group].

  A window of a recording: gu_T [R, C] is the gradient arriving at u_T,
  return_gu0 -> (gI, gu0) with gu0 [R, C] = dL/du0.  u0 is accepted for the signature it shares
  with neuron_backward; this neuron's backward does not read it.  With none of the three the call
  is the one it was (snnqp_lif_backward)."""
  h = _f32c(h)
  gs = None if gs is None else _f32c(gs)
  glogits = None if glogits is None else _f32c(glogits)
  _require_gpu(h, gs, glogits)
  T, C = h.shape[0], h.shape[-1]
  step = tuple(h.shape[1:])
  state = u0 is not None or gu_T is not None or return_gu0
  R = (math.prod(step) // C) if C and (T or state) else 0
  gI = torch.empty_like(h)
  if not state:
    if h.numel() == 0 and (gs is None) != (glogits is None) and (
        glogits is None or (group > 0 and C % group == 0)):
      return gI       # an empty upstream has no pointer for the library to tell gs from glogits by
    L.check(L.lib().snnqp_lif_backward(_ptr(h), _ptr(gs), _ptr(glogits), int(group), T, R, C,
                                       ctypes.byref(neuron.struct()), int(surrogate), _ptr(gI),
                                       _stream()))
    return gI
  _window_state("lif_backward", "u0", u0, step, h.device)
  gu_T = _window_state("lif_backward", "gu_T", gu_T, step, h.device)
  gu0 = torch.empty(step, dtype=torch.float32, device=h.device) if return_gu0 else None
  if h.numel() == 0:  # an empty upstream has no pointer to tell gs from glogits by; no step: gu0 = gu_T
    if (gs is None) == (glogits is None):
      raise ValueError("lif_backward: exactly one of gs / glogits")
    if gu0 is not None:
      gu0.zero_() if gu_T is None else gu0.copy_(gu_T.reshape(step))
  else:
    L.check(L.lib().snnqp_lif_backward_state(_ptr(h), _ptr(gs), _ptr(glogits), int(group), T, R, C,
                                             ctypes.byref(neuron.struct()), int(surrogate),
                                             _ptr(gu_T), _ptr(gI), _ptr(gu0), _stream()))
  return (gI, gu0) if return_gu0 else gI


def neuron_forward_save(x: torch.Tensor, neuron: Neuron, u0: Optional[torch.Tensor] = None,
                        return_state: bool = False):
  """lif_forward_save for the neurons with a parameter (PLIF, LIF; csrc/train_neuron.hip):
  currents float32 [T, ..., C] -> (h, s), the arithmetic of lif_forward for the same neuron.
  u0 and return_state as lif_forward_save's."""
  lib = L.lib()
  return _forward_save("neuron_forward_save", lib.snnqp_neuron_forward_save,
                       lib.snnqp_neuron_forward_save_state, x, neuron, u0, return_state)


def neuron_backward_splits(T: int, R: int, C: int) -> int:
  """The default number of row ranges of neuron_backward: shapes only."""
  rc = L.lib().snnqp_neuron_backward_splits(int(T), int(R), int(C))
  if rc < 0:
    L.check(rc)
  return rc


def neuron_backward_workspace_bytes(T: int, R: int, C: int, splits: int, kind: int) -> int:
  rc = L.lib().snnqp_neuron_backward_workspace_bytes(int(T), int(R), int(C), int(splits), int(kind))
  if rc < 0:
    L.check(rc)
  return rc


def neuron_backward(h: torch.Tensor, x: Optional[torch.Tensor], neuron: Neuron, surrogate: int,
                    gs: Optional[torch.Tensor] = None, glogits: Optional[torch.Tensor] = None,
                    group: int = 10, splits: Optional[int] = None,
                    u0: Optional[torch.Tensor] = None, gu_T: Optional[torch.Tensor] = None,
                    return_gu0: bool = False):
  """BPTT of the PLIF / LIF scan: h [T, R, C] and, for PLIF, the currents x the scan consumed ->
  (gI [T, R, C], gparam float64): gparam [1] = sum gh d for PLIF (the gradient of m), [C] =
  sum_{t,r} gh u_{t-1} for LIF (of the decays).  Upstream gs or glogits as lif_backward; the rows
  are cut into `splits` ranges summed in order (None: neuron_backward_splits).

  A window of a recording: u0 [R, C] is the membrane the forward started from --
  u_{-1} in the t = 0 term of both sums --, gu_T the gradient arriving at u_T, and return_gu0 ->
  (gI, gparam, gu0).  With none of the three the call is the one it was (snnqp_neuron_backward)."""
  h = _f32c(h)
  x = None if x is None or neuron.kind == L.NEURON_LIF else _f32c(x)
  gs = None if gs is None else _f32c(gs)
  glogits = None if glogits is None else _f32c(glogits)
  _require_gpu(h, x, gs, glogits)
  T, C = h.shape[0], h.shape[-1]
  step = tuple(h.shape[1:])
  state = u0 is not None or gu_T is not None or return_gu0
  R = (math.prod(step) // C) if C and (T or state) else 0
  if neuron.kind == L.NEURON_PARAMETRIC_LEAKY_IF and h.numel():
    if x is None or tuple(x.shape) != tuple(h.shape):
      raise ValueError("neuron_backward: PLIF needs the scan's currents x, shaped like h")
  if splits is None:
    splits = neuron_backward_splits(T, R, C)
  # (another kind has no workspace to size: the call below refuses it, naming its own entry point)
  known = neuron.kind in (L.NEURON_PARAMETRIC_LEAKY_IF, L.NEURON_LIF)
  nbytes = neuron_backward_workspace_bytes(T, R, C, splits, neuron.kind) if known else 0
  gI = torch.empty_like(h)
  gparam = torch.empty((C if neuron.kind == L.NEURON_LIF else 1,), dtype=torch.float64, device=h.device)
  if not state:
    if h.numel() == 0 and (gs is None) != (glogits is None) and (
        glogits is None or (group > 0 and C % group == 0)):
      return gI, gparam.zero_()   # an empty upstream has no pointer to tell gs from glogits by
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=h.device)
    L.check(L.lib().snnqp_neuron_backward(_ptr(h), _ptr(x), _ptr(gs), _ptr(glogits), int(group), T, R, C,
                                          ctypes.byref(neuron.struct()), int(surrogate), int(splits),
                                          _ptr(gI), _ptr(gparam), _ptr(ws), nbytes, _stream()))
    return gI, gparam
  u0 = _window_state("neuron_backward", "u0", u0, step, h.device)
  gu_T = _window_state("neuron_backward", "gu_T", gu_T, step, h.device)
  gu0 = torch.empty(step, dtype=torch.float32, device=h.device) if return_gu0 else None
  if h.numel() == 0:  # an empty upstream has no pointer to tell gs from glogits by; no step: gu0 = gu_T
    if (gs is None) == (glogits is None):
      raise ValueError("neuron_backward: exactly one of gs / glogits")
    gparam.zero_()
    if gu0 is not None:
      gu0.zero_() if gu_T is None else gu0.copy_(gu_T.reshape(step))
  else:
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=h.device)
    L.check(L.lib().snnqp_neuron_backward_state(
        _ptr(h), _ptr(x), _ptr(u0), _ptr(gs), _ptr(glogits), int(group), T, R, C,
        ctypes.byref(neuron.struct()), int(surrogate), int(splits), _ptr(gu_T), _ptr(gI), _ptr(gu0),
        _ptr(gparam), _ptr(ws), nbytes, _stream()))
  return (gI, gparam, gu0) if return_gu0 else (gI, gparam)


def dense_weight_grad(x: torch.Tensor, gI: torch.Tensor) -> torch.Tensor:
  """x [M, K], gI [M, N] -> x^T gI [K, N] (float32 MFMA, one fixed reduction order)."""
  x, gI = _f32c(x), _f32c(gI)
  _require_gpu(x, gI)
  M, K = x.shape
  N = gI.shape[1]
  assert gI.shape[0] == M
  gw = torch.empty((K, N), dtype=torch.float32, device=x.device)
  L.check(L.lib().snnqp_dense_weight_grad(_ptr(x), _ptr(gI), M, K, N, _ptr(gw), _stream()))
  return gw


def dense_input_grad(gI: torch.Tensor, w: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
  """gI [M, N], w [K, N] -> (gI w^T) * mask [M, K]."""
  gI, w = _f32c(gI), _f32c(w)
  mask = None if mask is None else _f32c(mask)
  _require_gpu(gI, w, mask)
  M, N = gI.shape
  K = w.shape[0]
  assert w.shape[1] == N and (mask is None or tuple(mask.shape) == (M, K))
  gx = torch.empty((M, K), dtype=torch.float32, device=gI.device)
  L.check(L.lib().snnqp_dense_input_grad(_ptr(gI), _ptr(w), _ptr(mask), M, K, N, _ptr(gx),
                                         _stream()))
  return gx


# ---------------------------------------------------------------------------
# training of the conv blocks (csrc/train_conv.hip)
# ---------------------------------------------------------------------------


def conv_grad_splits(geom: ConvGeom, NB: int) -> int:
  """The default number of r ranges of conv_weight_grad for NB images: shapes only, 1..64."""
  g = geom.struct()
  rc = L.lib().snnqp_conv_grad_splits(ctypes.byref(g), int(NB))
  if rc < 0:
    L.check(rc)
  return rc


def conv_weight_grad_workspace_bytes(geom: ConvGeom, splits: int) -> int:
  g = geom.struct()
  rc = L.lib().snnqp_conv_weight_grad_workspace_bytes(ctypes.byref(g), int(splits))
  if rc < 0:
    L.check(rc)
  return rc


def conv_weight_grad(x: torch.Tensor, gI: torch.Tensor, geom: ConvGeom,
                     splits: Optional[int] = None) -> torch.Tensor:
  """x [NB, H, W, Cin], gI [NB, OH, OW, Cout] -> gw HWIO [KH, KW, Cin, Cout]: the r-ascending
  chain over r = (n, oh, ow), cut into `splits` ranges summed in order (None: conv_grad_splits)."""
  x, gI = _f32c(x), _f32c(gI)
  _require_gpu(x, gI)
  NB = x.shape[0]
  g = geom.struct()
  if splits is None:
    splits = conv_grad_splits(geom, NB)
  nbytes = conv_weight_grad_workspace_bytes(geom, splits)
  OH, OW = geom.out_hw()
  assert tuple(x.shape) == (NB, geom.H, geom.W, geom.Cin), (tuple(x.shape), geom)
  assert tuple(gI.shape) == (NB, OH, OW, geom.Cout), (tuple(gI.shape), geom)
  ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
  gw = torch.empty((geom.KH, geom.KW, geom.Cin, geom.Cout), dtype=torch.float32, device=x.device)
  L.check(L.lib().snnqp_conv_weight_grad(_ptr(x), _ptr(gI), NB, ctypes.byref(g), int(splits),
                                         _ptr(ws), _ptr(gw), _stream()))
  return gw


def conv_weight_grad_f64(x: torch.Tensor, gI: torch.Tensor, geom: ConvGeom) -> torch.Tensor:
  """conv_weight_grad with the chain over r in float64 (ranges of about 1024 rows summed in order,
  one rounding to float32): for a layer whose gradient cancels too far for a float32 chain."""
  x, gI = _f32c(x), _f32c(gI)
  _require_gpu(x, gI)
  NB = x.shape[0]
  g = geom.struct()
  nbytes = L.lib().snnqp_conv_weight_grad_f64_workspace_bytes(ctypes.byref(g), int(NB))
  if nbytes < 0:
    L.check(nbytes)
  OH, OW = geom.out_hw()
  assert tuple(x.shape) == (NB, geom.H, geom.W, geom.Cin), (tuple(x.shape), geom)
  assert tuple(gI.shape) == (NB, OH, OW, geom.Cout), (tuple(gI.shape), geom)
  ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
  gw = torch.empty((geom.KH, geom.KW, geom.Cin, geom.Cout), dtype=torch.float32, device=x.device)
  L.check(L.lib().snnqp_conv_weight_grad_f64(_ptr(x), _ptr(gI), NB, ctypes.byref(g), _ptr(ws),
                                             _ptr(gw), _stream()))
  return gw


def conv_input_grad(gI: torch.Tensor, w: torch.Tensor, geom: ConvGeom) -> torch.Tensor:
  """gI [NB, OH, OW, Cout], w HWIO -> gx [NB, H, W, Cin], the chain over r = (kh, kw, co)."""
  gI, w = _f32c(gI), _f32c(w)
  _require_gpu(gI, w)
  NB = gI.shape[0]
  g = geom.struct()
  conv_grad_splits(geom, 0)                    # refuses the geometry before any shape is used
  OH, OW = geom.out_hw()
  assert tuple(gI.shape) == (NB, OH, OW, geom.Cout), (tuple(gI.shape), geom)
  assert tuple(w.shape) == (geom.KH, geom.KW, geom.Cin, geom.Cout), (tuple(w.shape), geom)
  gx = torch.empty((NB, geom.H, geom.W, geom.Cin), dtype=torch.float32, device=gI.device)
  L.check(L.lib().snnqp_conv_input_grad(_ptr(gI), _ptr(w), NB, ctypes.byref(g), _ptr(gx),
                                        _stream()))
  return gx


def maxpool2x2_backward(s: torch.Tensor, gp: torch.Tensor) -> torch.Tensor:
  """s [..., H, W, C] the pool's float32 input, gp [..., H/2, W/2, C] -> gs like s: gp to the
  first maximum of each window in row-major order, 0 elsewhere."""
  s, gp = _f32c(s), _f32c(gp)
  _require_gpu(s, gp)
  H, W, C = s.shape[-3:]
  assert tuple(gp.shape) == tuple(s.shape[:-3]) + (H // 2, W // 2, C), (s.shape, gp.shape)
  NB = s.numel() // (H * W * C) if H * W * C else 0
  gs = torch.empty_like(s)
  L.check(L.lib().snnqp_maxpool2x2_backward(_ptr(s), _ptr(gp), NB, H, W, C, _ptr(gs), _stream()))
  return gs


# ---------------------------------------------------------------------------
# training of a conv block with rematerialisation (csrc/train_remat.hip)
# ---------------------------------------------------------------------------


def bn_lif_forward(cur: torch.Tensor, mean: torch.Tensor, mul: torch.Tensor, bias: torch.Tensor,
                   neuron: Neuron, u0: Optional[torch.Tensor] = None, want_h: bool = True,
                   want_s: bool = True, return_state: bool = False):
  """The batch-statistics normalisation and lif_forward_save in one pass: raw
  currents cur float32 [T, ..., C], per-step mean and multiplier [T, C] (conv_train.bn_multiplier),
  bias [C] -> (h, s) float32 like cur, from u0 [..., C] (None: zeros); h or s is None where it is
  not wanted, and is then not written.  return_state -> (h, s, u_T).  The normalised currents are
  never written.  multi_step_LIF only."""
  cur, mean, mul, bias = _f32c(cur), _f32c(mean), _f32c(mul), _f32c(bias)
  _require_gpu(cur, mean, mul, bias)
  T, C = cur.shape[0], cur.shape[-1]
  step = tuple(cur.shape[1:])
  if tuple(mean.shape) != (T, C) or tuple(mul.shape) != (T, C) or tuple(bias.shape) != (C,):
    raise ValueError("bn_lif_forward: mean and mul must be [%d, %d] and bias [%d], got %s, %s, %s"
                     % (T, C, C, tuple(mean.shape), tuple(mul.shape), tuple(bias.shape)))
  R = (math.prod(step) // C) if C else 0
  u0 = _window_state("bn_lif_forward", "u0", u0, step, cur.device)
  h = torch.empty_like(cur) if want_h else None
  s = torch.empty_like(cur) if want_s else None
  u_out = torch.empty(step, dtype=torch.float32, device=cur.device) if return_state else None
  L.check(L.lib().snnqp_bn_lif_forward_state(
      _ptr(cur), _ptr(mean), _ptr(mul), _ptr(bias), T, R, C, ctypes.byref(neuron.struct()),
      _ptr(u0), _ptr(u_out), _ptr(h), _ptr(s), _stream()))
  return (h, s, u_out) if return_state else (h, s)


def maxpool2x2_backward_h(h: torch.Tensor, v_threshold: float, gp: torch.Tensor) -> torch.Tensor:
  """maxpool2x2_backward with the pool's input s = ((h - v_threshold) >= 0) read from the scan's
  h [..., H, W, C] by the forward's own compare: no spike raster is written."""
  h, gp = _f32c(h), _f32c(gp)
  _require_gpu(h, gp)
  H, W, C = h.shape[-3:]
  assert tuple(gp.shape) == tuple(h.shape[:-3]) + (H // 2, W // 2, C), (h.shape, gp.shape)
  NB = h.numel() // (H * W * C) if H * W * C else 0
  gs = torch.empty_like(h)
  L.check(L.lib().snnqp_maxpool2x2_backward_h(_ptr(h), float(v_threshold), _ptr(gp), NB, H, W, C,
                                              _ptr(gs), _stream()))
  return gs


# ---------------------------------------------------------------------------
# training of CextNet's gated stages (csrc/train_gate.hip)
# ---------------------------------------------------------------------------


def _gate_stage_shapes(x, gate, gp):
  H, W, C = x.shape[-3:]
  lead = tuple(x.shape[:-3])
  assert tuple(gate.shape) == lead + (C,), (x.shape, gate.shape)
  assert tuple(gp.shape) == lead + (H // 2, W // 2, C), (x.shape, gp.shape)
  NB = x.numel() // (H * W * C) if H * W * C else 0
  return NB, H, W, C, lead


def gate_pool_grad_gate(x: torch.Tensor, gate: torch.Tensor, gp: torch.Tensor) -> torch.Tensor:
  """x [..., H, W, C], gate [..., C], gp [..., H/2, W/2, C] -> ggate [..., C] of
  p = maxpool2x2(x * gate): sum over the windows of gp * x at the first maximum of x * gate, one
  fmaf chain in ascending (ph, pw)."""
  x, gate, gp = _f32c(x), _f32c(gate), _f32c(gp)
  _require_gpu(x, gate, gp)
  NB, H, W, C, lead = _gate_stage_shapes(x, gate, gp)
  ggate = torch.empty(lead + (C,), dtype=torch.float32, device=x.device)
  L.check(L.lib().snnqp_gate_pool_grad_gate(_ptr(x), _ptr(gate), _ptr(gp), NB, H, W, C, _ptr(ggate),
                                            _stream()))
  return ggate


def gate_pool_grad_input(x: torch.Tensor, gate: torch.Tensor, gp: torch.Tensor,
                         gm: torch.Tensor) -> torch.Tensor:
  """-> gx like x: gp * gate routed to the first maximum of x * gate in each window, plus
  gm [..., C] / (H W), the gradient through spatial_mean(x)."""
  x, gate, gp, gm = _f32c(x), _f32c(gate), _f32c(gp), _f32c(gm)
  _require_gpu(x, gate, gp, gm)
  NB, H, W, C, lead = _gate_stage_shapes(x, gate, gp)
  assert tuple(gm.shape) == lead + (C,), (x.shape, gm.shape)
  gx = torch.empty_like(x)
  L.check(L.lib().snnqp_gate_pool_grad_input(_ptr(x), _ptr(gate), _ptr(gp), _ptr(gm), NB, H, W, C,
                                             _ptr(gx), _stream()))
  return gx


# ---------------------------------------------------------------------------
# magnitude pruning (csrc/prune.hip)
# ---------------------------------------------------------------------------


def magnitude_prune(w: torch.Tensor, mask: torch.Tensor, k: int) -> torch.Tensor:
  """Prunes `mask` in place up to k zeros and returns it: with m entries already pruned
  (mask == 0), the k - m unpruned entries smallest by the key bits(|w|) read as uint32, ties by
  ascending flat index, get mask = 0; k <= m writes nothing, and no other value of `mask` is
  touched.  w, mask: float32 of one shape (flat or shaped), mask contiguous.  On CUDA tensors one
  launch sequence on the current stream (snnqp_magnitude_prune: no host read, no sync; the
  workspace comes from torch's allocator and is not kept); on CPU tensors the same rule in torch
  ops (a stable sort on the key), for the host logic of the training loop.  Either way `mask`
  counts as written in place (its version moves)."""
  if w.dtype != torch.float32 or mask.dtype != torch.float32:
    raise TypeError("magnitude_prune: float32 tensors (w %s, mask %s)" % (w.dtype, mask.dtype))
  if tuple(w.shape) != tuple(mask.shape) or w.device != mask.device:
    raise ValueError("magnitude_prune: w %s on %s, mask %s on %s" % (tuple(w.shape), w.device, tuple(mask.shape),
                                                                     mask.device))
  if not mask.is_contiguous():
    raise ValueError("magnitude_prune: mask is written in place and must be contiguous")
  n, k = mask.numel(), int(k)
  if not 0 <= k <= n:
    raise ValueError("magnitude_prune: k = %d outside [0, n = %d]" % (k, n))
  w = w.detach().contiguous()
  m_ = mask.detach()
  if not mask.is_cuda:
    if k == 0:
      return mask
    key = w.reshape(-1).view(torch.int32) & 0x7FFFFFFF             # non-negative: int32 order = uint32 order
    flat = m_.reshape(-1)
    idx = torch.nonzero((flat.view(torch.int32) & 0x7FFFFFFF) != 0).reshape(-1)       # ascending
    more = k - (n - idx.numel())
    if more > 0:
      order = torch.sort(key[idx], stable=True).indices[:more]
      flat[idx[order]] = 0.0
    return mask
  nbytes = L.lib().snnqp_magnitude_prune_workspace_bytes(n)
  if nbytes < 0:
    L.check(nbytes)
  ws = torch.empty(nbytes // 4, dtype=torch.int32, device=mask.device)
  with torch.cuda.device(mask.device):
    L.check(L.lib().snnqp_magnitude_prune(_ptr(w), _ptr(m_), n, k, _ptr(ws), nbytes, _stream()))
  # the library wrote through the pointer: what caches by tensor version (packing.get_packed, the
  # channel and head plans) has to see an in-place write, as it does after a torch op
  torch.autograd.graph.increment_version(mask)
  return mask
