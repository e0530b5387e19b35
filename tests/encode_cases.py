"""Plain numpy restatement of snnqp_rate_encode's contract (include/snnqp.h) as a reference --
the hash, the key, the decision per element, the bit-packing, the threshold table --, written from
the contract and not from the package, and the small learnable image fixture of the loop tests.
Nothing here needs a GPU."""
import math

import numpy as np

U32 = np.uint32
TOP = 2 ** 32
COUNT_MAX = 15


def fmix32(h):
  """The murmur3 finaliser on uint32 arrays (wrapping arithmetic)."""
  h = np.asarray(h, dtype=np.uint64) & 0xFFFFFFFF
  h ^= h >> 16
  h = (h * 0x85EBCA6B) & 0xFFFFFFFF
  h ^= h >> 13
  h = (h * 0xC2B2AE35) & 0xFFFFFFFF
  h ^= h >> 16
  return h.astype(U32)


def fmix32_scalar(h: int) -> int:
  """The same on one Python int: a second implementation to hold the first against."""
  h &= 0xFFFFFFFF
  h ^= h >> 16
  h = (h * 0x85EBCA6B) % TOP
  h ^= h >> 13
  h = (h * 0xC2B2AE35) % TOP
  h ^= h >> 16
  return h


def row_key(seed, draw, sample_id):
  """c = fmix32(fmix32(seed ^ fmix32(draw)) ^ sample_id), all modulo 2^32."""
  seed, draw = int(seed) % TOP, int(draw) % TOP
  inner = fmix32(U32(seed) ^ fmix32(U32(draw)))
  return fmix32(inner ^ (np.asarray(sample_id, dtype=np.uint64) & 0xFFFFFFFF).astype(U32))


def hashes(seed, draw, sample_id, T, K):
  """u of every (row, t, k): uint32 [B, T, K]."""
  c = row_key(seed, draw, np.asarray(sample_id).reshape(-1))
  e = (np.arange(T, dtype=np.uint64)[:, None] * K + np.arange(K, dtype=np.uint64)[None, :]).astype(U32)
  return fmix32(c[:, None, None] ^ e[None])


def rate_encode_reference(images, sample, sample_id, T, table, kind, seed, draw):
  """uint8 [B, T, K]: images uint8 [S, K], table uint32 [256, 16], kind "bernoulli" | "poisson".
  An entry of 2^32 - 1 stands for 2^32 (the comparisons are made in 64 bits)."""
  images = np.asarray(images).reshape(np.asarray(images).shape[0], -1)
  sample = np.asarray(sample, dtype=np.int64).reshape(-1)
  B, K = sample.shape[0], images.shape[1]
  u = hashes(seed, draw, sample_id, T, K).astype(np.int64)
  th = np.asarray(table, dtype=np.int64)
  th = np.where(th == TOP - 1, TOP, th)
  rows = th[images[sample].astype(np.int64)]                            # [B, K, 16]
  if kind == "bernoulli":
    return (u < rows[:, None, :, 0]).astype(np.uint8)
  assert kind == "poisson", kind
  out = np.zeros((B, T, K), np.uint8)
  for j in range(COUNT_MAX):
    out += (u >= rows[:, None, :, j]).astype(np.uint8)
  return out


def pack_bits_reference(x):
  """0 / 1 [..., K] -> int32 [..., ceil(K / 32)]: element k in bit (k & 31) of word (k >> 5)."""
  x = np.asarray(x)
  K = x.shape[-1]
  words = (K + 31) // 32
  padded = np.zeros(x.shape[:-1] + (words * 32,), np.uint64)
  padded[..., :K] = x != 0
  w = (padded.reshape(x.shape[:-1] + (words, 32)) << np.arange(32, dtype=np.uint64)).sum(-1)
  return w.astype(U32).view(np.int32)


def rates(gain=1.0, mean=0.0, std=1.0):
  return [max(0.0, gain * ((v / 255.0 - mean) / std)) for v in range(256)]


def table_reference(kind, gain=1.0, mean=0.0, std=1.0):
  """An independent float64 builder, value by value in Python floats: uint32 [256, 16]."""
  out = np.zeros((256, 16), np.uint64)
  for v, r in enumerate(rates(gain, mean, std)):
    if kind == "bernoulli":
      out[v, 0] = min(math.floor(min(r, 1.0) * TOP), TOP - 1)
      continue
    term = math.exp(-r)
    cdf = term
    for j in range(COUNT_MAX):
      if j > 0:
        term *= r / j
        cdf += term
      out[v, j] = min(math.floor(cdf * TOP), TOP - 1)
  return out.astype(U32)


def truncated_mass_reference(r: float) -> float:
  """P(X > 15; r) by direct summation of the tail's terms (they fall off faster than geometrically
  once j > r), without forming 1 - cdf."""
  if r == 0.0:
    return 0.0
  log_term = -r + (COUNT_MAX + 1) * math.log(r) - math.lgamma(COUNT_MAX + 2)
  term = math.exp(log_term)
  total, j = 0.0, COUNT_MAX + 1
  while term > 1e-320 and j < 10000:
    total += term
    j += 1
    term *= r / j
  return total


def constant_table(threshold0, rest=0):
  """A table with the same row for every pixel value."""
  t = np.full((256, 16), rest, np.uint64)
  t[:, 0] = threshold0
  t[:, 15] = 0
  return t.astype(U32)


# ---- the learnable fixture: 8 x 8 one-channel images, left half bright / right half bright ---------

SIDE, CLASSES, HIDDEN, T_STEPS = 8, 2, 32, 8
N_TRAIN, N_TEST, BATCH = 64, 32, 16


def make_images(seed, n):
  """{"image": uint8 [n, 8, 8], "label": int8 [n]}: class c's bright half is columns 4c .. 4c + 3
  (200 +- 40), the other half dark (20 +- 20), noise per image and pixel."""
  rng = np.random.Generator(np.random.PCG64(seed))
  labels = (np.arange(n) % CLASSES).astype(np.int8)
  img = rng.integers(0, 41, (n, SIDE, SIDE))
  for i, y in enumerate(labels):
    img[i, :, 4 * y:4 * y + 4] = rng.integers(160, 241, (SIDE, 4))
  return {"image": img.astype(np.uint8), "label": labels}


def sources():
  return make_images(11, N_TRAIN), make_images(12, N_TEST)


def make_config(**kw):
  """The loop's config on the fixture: DenseSNN (hidden 32, float weights: config C1's shape), T = 8,
  Poisson counts at gain 2, adam at 0.05, batches of 16 (4 steps an epoch), a record per step and a
  checkpoint per epoch.  With these the float64 replay (reference_losses) takes the loss from 0.5 --
  the silent net model.init gives -- to below 0.01 within 3 epochs, from either of two initial
  draws; at learning rate 0.01 it had barely moved by then (0.37 .. 0.22), and Bernoulli spikes at
  gain 1 left the net silent for the whole first two epochs."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import synthetic as syn
  cfg = syn.make_config(bits=8, prune_percentage=-1.0, hidden=HIDDEN, dropout=1.0)
  cfg.model, cfg.num_classes, cfg.num_frames = "DenseSNN", CLASSES, T_STEPS
  cfg.encoding = nn.ConfigDict(kind="poisson", gain=2.0)
  cfg.batch_size, cfg.eval_batch_size, cfg.feed_format, cfg.seed = BATCH, BATCH, "u8", 5
  cfg.optimizer, cfg.learning_rate, cfg.weight_decay, cfg.smoothing = "adam", 0.05, 0.0, 0.0
  cfg.num_epochs, cfg.warmup_epochs, cfg.num_train_steps, cfg.steps_per_eval = 3, 1, -1, -1
  cfg.log_every_steps, cfg.checkpoint_every_epochs = 1, 1
  for k, v in kw.items():
    cfg[k] = v
  return cfg


TAU, V_TH, V_RESET = 2.0, 1.0, 0.0          # synthetic.make_config's neuron: multi_step_LIF(atan, tau 2)


def _saved_forward(params, x_bt):
  """The spikes and pre-reset potentials TorchDenseSNN64 replays (h1, s1, h2, s2, float32
  [T, B, N]), from a float64 forward of the current float32 weights (no dropout, no quantisation:
  a = c = -1 and all-one masks, as model.init leaves them)."""
  x = np.swapaxes(np.asarray(x_bt, np.float64), 0, 1)
  saved = []
  for i in (0, 1):
    leaf = params["QuantDense_%d" % i]
    assert float(np.asarray(leaf["DuQ_0"]["a"]).reshape(-1)[0]) == -1.0
    w = np.asarray(leaf["kernel"], np.float64)
    u = np.zeros((x.shape[1], w.shape[1]))
    hs, ss = [], []
    for t in range(x.shape[0]):
      h = u + (x[t] @ w - (u - V_RESET)) / TAU
      s = (h - V_TH >= 0).astype(np.float64)
      u = np.where(s != 0, V_RESET, h)
      hs.append(h)
      ss.append(s)
    x = np.stack(ss)
    saved += [np.stack(hs).astype(np.float32), x.astype(np.float32)]
  return saved


def reference_losses(params, batches, lr_fn):
  """Loss per step of tests/train_reference.TorchDenseSNN64 trained on `batches` ([(x uint8 [B, T, K],
  labels)]) with Adam (b1 0.9, b2 0.999, eps 1e-8, in float64) at lr_fn(step), the way
  train_loop_cases.reference_losses replays the conv fixture: says whether the fixture can be
  learnt at all."""
  import torch
  from snnquantprune_amd import train_utils as tu
  from tests import train_reference as tr
  params = {k: dict(leaf, kernel=np.array(leaf["kernel"], np.float32)) for k, leaf in params.items()}
  moments, losses = {}, []
  for step, (x, y) in enumerate(batches):
    h1, s1, h2, s2 = _saved_forward(params, x)
    m = tr.TorchDenseSNN64(params, TAU, V_TH, V_RESET, "atan")
    ones0, ones1 = np.ones(x.shape), np.ones(s1.shape)
    loss = tu.mse_loss(m.forward(x, ones0, ones1, h1, s1, h2, s2), torch.from_numpy(np.asarray(y, np.int64)))
    loss.backward()
    losses.append(float(loss.detach()))
    lr, t = lr_fn(step), step + 1
    for i, (g, _, _) in m.grads().items():
      mu, nu = moments.setdefault(i, (np.zeros_like(g), np.zeros_like(g)))
      mu[...] = 0.9 * mu + 0.1 * g
      nu[...] = 0.999 * nu + 0.001 * g * g
      upd = lr * (mu / (1 - 0.9 ** t)) / (np.sqrt(nu / (1 - 0.999 ** t)) + 1e-8)
      leaf = params["QuantDense_%d" % i]
      leaf["kernel"] = (np.asarray(leaf["kernel"], np.float64) - upd).astype(np.float32)
  return losses


def plan_batches(source, cfg, steps, train, rank=0, world=1, skip=0):
  """The first `steps` batches of the split as the plan draws them, encoded by the reference:
  [(uint8 [B, T, K], labels int64, indices, draw)]."""
  from snnquantprune_amd import input_pipeline as ip
  n = source["label"].shape[0] // world
  lo = rank * n
  plan = ip.ImagePlan(cfg, source["image"].shape[1:], n, train, rank, world)
  enc = cfg.encoding
  table = table_reference(enc.get("kind", "poisson"), enc.get("gain", 1.0), enc.get("mean", 0.0), enc.get("std", 1.0))
  images = source["image"][lo:lo + n]
  it = plan.batches(skip)
  out = []
  for _ in range(steps):
    idx, ids, draw = next(it)
    x = rate_encode_reference(images, idx, ids, plan.T, table, enc.get("kind", "poisson"), cfg.seed, draw)
    out.append((x, source["label"][lo:lo + n][idx].astype(np.int64), idx, draw))
  return out
