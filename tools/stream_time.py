"""What streaming inference costs:

  head   config C2's head (2048 -> 512 -> 110, B = 256) over windows of 1, 5 and 20 steps: ms per window of
         the stateful one-launch head (DenseSNN.apply(u_state=...)) against the path a streaming caller
         had before it -- two ops.dense_lif_forward calls with u0 / want_u and ops.vote --, eager (host
         clock around N windows, ending in a synchronise) and as a replayed hipGraph (device events).
  conv   ConvDenseSNN at config C3's geometry (128 x 128 frames, 128 channels, EV1 frames): ms per
         step of the streaming call (uncompacted, every block carrying its membranes) in windows of 5
         and 20 steps against the whole-run call of 20 steps (compacted, no state).

Every pair is timed alternately, `--reps` times; the table holds the median and the spread (max - min)
of each.  Needs the GPU: there is no fallback.

   python tools/stream_time.py [--reps 7] [--windows 300] [--conv-batch 16] [--out profiles/FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from snnquantprune_amd import _lib as L, linen as nn, models, ops, synthetic as syn   # noqa: E402


def _eager_ms(fn, n):
  torch.cuda.synchronize()
  t = time.perf_counter()
  for _ in range(n):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t) * 1e3 / n


def _event_ms(fn, n):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  a.record()
  for _ in range(n):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / n


def _graph_of(fn, dev):
  """fn recorded into a hipGraph (its launches touch fixed buffers only) -> replay()."""
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  graph = torch.cuda.CUDAGraph()
  keep, outer = [], ops._CAPTURE_KEEP
  with torch.cuda.stream(side):
    for _ in range(2):
      fn()
    side.synchronize()
    ops._CAPTURE_KEEP = keep
    try:
      with torch.cuda.graph(graph, stream=side):
        fn()
    finally:
      ops._CAPTURE_KEEP = outer
  torch.cuda.current_stream(dev).wait_stream(side)
  graph._keep = keep
  return graph.replay


def _summary(samples):
  return {"median_ms": statistics.median(samples), "spread_ms": max(samples) - min(samples), "samples_ms": samples}


def head_table(dev, reps, n):
  B, K, N1, N2 = 256, 2048, 512, 110
  cfg = syn.make_config(bits=8, prune_percentage=0.5, hidden=N1)
  model = models.DenseSNN(num_classes=11, config=cfg)
  tree = syn.dense_net_variables(K, N1, N2, True, 0.5)
  variables = nn.tree_from_numpy(tree, dev)
  # the per-block path's operands, packed as SpikingBlock packs them
  from snnquantprune_amd import packing
  from snnquantprune_amd.quant import QuantDesc

  def weight(leaf, n):
    a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
    pk = packing.PackedKernel(torch.from_numpy(leaf["kernel"]).to(dev), QuantDesc(L.Q_DUQ, 8, a, c, 127.0, c),
                              torch.from_numpy(leaf["prune_0"]["mask"]).to(dev))
    return pk.int_weight_mfma((n + 31) // 32 * 32)
  w1, w2 = weight(tree["params"]["QuantDense_0"], N1), weight(tree["params"]["QuantDense_1"], N2)
  nrn = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)
  rows = []
  for tw in (1, 5, 20):
    x = (torch.rand((B, tw, K), device=dev) < 0.1).to(torch.uint8)
    state = models.StreamState()

    def head():
      return model.apply(variables, x, trgt=None, train=False, rng=None, u_state=state)
    u = [torch.zeros((B, N1), device=dev), torch.zeros((B, N2), device=dev)]
    ug = [torch.zeros((B, N1), device=dev), torch.zeros((B, N2), device=dev)]     # the recorded path's own

    def per_block(u=u, fixed=False):
      """eager: the caller keeps the tensors it gets back; recorded: it copies them to fixed buffers"""
      n1, s1 = ops.dense_lif_forward(x, w1, K, N1, nrn, u0=u[0], want_u=True, packed_out=True, time_major=False)
      n2, s2 = ops.dense_lif_forward(s1, w2, N1, N2, nrn, u0=u[1], want_u=True, packed_out=True)
      if fixed:
        u[0].copy_(n1)
        u[1].copy_(n2)
      else:
        u[0], u[1] = n1, n2
      return ops.vote(s2, 10)
    head(); per_block()
    state.reset()
    u[0], u[1] = torch.zeros_like(u[0]), torch.zeros_like(u[1])
    a, b = head()[0], per_block()
    torch.cuda.synchronize()
    same = bool(torch.equal(a, b)) and bool(torch.equal(state.membranes[0], u[0])) and bool(torch.equal(state.membranes[1], u[1]))
    step = nn.capture(model, variables, x, trgt=None, train=False, rng=None, u_state=state)
    replay_pb = _graph_of(lambda: per_block(ug, True), dev)
    t = {k: [] for k in ("head_eager", "per_block_eager", "head_graph", "per_block_graph")}
    for _ in range(reps):
      t["head_eager"].append(_eager_ms(head, n))
      t["per_block_eager"].append(_eager_ms(per_block, n))
      t["head_graph"].append(_event_ms(step, n))
      t["per_block_graph"].append(_event_ms(replay_pb, n))
    step.close()
    row = {"window": tw, "B": B, "same_bits": same}
    row.update({k: _summary(v) for k, v in t.items()})
    rows.append(row)
    print(json.dumps(row), flush=True)
  return rows


def conv_table(dev, reps, B):
  hw, T = 128, 20
  cfg = syn.make_config(bits=4, prune_percentage=0.9)
  model = models.ConvDenseSNN(num_classes=11, config=cfg)
  variables = nn.tree_from_numpy(syn.conv_net_variables(hw=hw, prune_p=0.9, random_bn=True), dev)
  frames = (torch.rand((B, T, hw, hw, 2), device=dev) < 0.1).to(torch.uint8)
  whole_x = ops.pack_frames(frames, L.EV1)

  def whole():
    return model.apply(variables, whole_x, trgt=None, train=False, rng=None)
  rows = []
  for tw in (5, 20):
    wins = [ops.pack_frames(frames[:, t0:t0 + tw].contiguous(), L.EV1) for t0 in range(0, T, tw)]
    state = models.StreamState()

    def stream():
      for w in wins:
        model.apply(variables, w, trgt=None, train=False, rng=None, u_state=state)
    whole(); stream()
    state.reset()
    stream()
    same = bool(torch.equal(state.logits(10), whole()[0]))
    t = {"stream": [], "whole_run": []}
    for _ in range(reps):
      t["stream"].append(_eager_ms(stream, 3) / T)
      t["whole_run"].append(_eager_ms(whole, 3) / T)
    row = {"window": tw, "B": B, "T": T, "same_logits": same, "unit": "ms per time step"}
    row.update({k: _summary(v) for k, v in t.items()})
    rows.append(row)
    print(json.dumps(row), flush=True)
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=7)
  ap.add_argument("--windows", type=int, default=300)
  ap.add_argument("--conv-batch", type=int, default=16)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "stream_time.py measures on the GPU"
  L.require_product_build()
  dev = torch.device("cuda:0")
  out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "windows_per_sample": args.windows,
         "head": head_table(dev, args.reps, args.windows), "conv": conv_table(dev, args.reps, args.conv_batch)}
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump(out, f, indent=1)
      f.write("\n")


if __name__ == "__main__":
  main()
