"""Shared by the GPU tests of the training paths: running a model's training forward on
gradient-carrying copies of its parameters (the model-level files), and framed device buffers
for calling one kernel at a time (the kernel-level files)."""
import numpy as np
import torch

F32 = np.float32
PAD = 4096


def _np(t):
  return t.detach().cpu().numpy()


# ---- model level -----------------------------------------------------------------------------------

def _leaves(tree):
  return {k: (_leaves(t) if isinstance(t, dict) else t.detach().clone().requires_grad_(True))
          for k, t in tree.items()}


def _run_train(model, variables, x, rng=0, batch_stats=True):
  """One training forward on fresh leaves -> (params, logits, sown values, new batch_stats);
  batch_stats=False (DenseSNN has none): an empty collection in, and no fourth result."""
  params = _leaves(variables["params"])
  mutable = ["intermediates", "batch_stats"] if batch_stats else ["intermediates"]
  (logits, _), mut = model.apply(
      {"params": params, "batch_stats": variables["batch_stats"] if batch_stats else {}}, x,
      train=True, rng=rng, mutable=mutable)
  inter = {k: v[0] for k, v in mut["intermediates"].items()}
  return (params, logits, inter, mut["batch_stats"]) if batch_stats else (params, logits, inter)


def _grad_tree(params, prefix=()):
  out = {}
  for k, t in params.items():
    if isinstance(t, dict):
      out.update(_grad_tree(t, prefix + (k,)))
    else:
      out[prefix + (k,)] = None if t.grad is None else _np(t.grad)
  return out


# ---- kernel level ----------------------------------------------------------------------------------

def mixed(rng, shape):
  """Mixed magnitudes, so that the order of a float32 sum shows in its bits."""
  return (rng.standard_normal(shape) * 2.0 ** rng.integers(-6, 7, shape)).astype(F32)


def _framed(dev, a, fill, pad=PAD):
  """A device copy of `a` with a frame of `fill`, `pad` elements before and after it: (whole,
  view).  An odd pad also leaves the view only 4-byte aligned."""
  whole = torch.full((a.size + 2 * pad,), float(fill), dtype=torch.float32, device=dev)
  view = whole[pad:pad + a.size].view(a.shape)
  view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
  return whole, view


def _frame_untouched(whole, n, fill, pad=PAD):
  edge = torch.cat([whole[:pad], whole[pad + n:]])
  return bool(torch.isnan(edge).all()) if np.isnan(fill) else bool((edge == fill).all())
