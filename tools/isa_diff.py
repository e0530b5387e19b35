"""Two device-only assembly files (hipcc ... --cuda-device-only -S, as tools/kernel_regs.py compiles
them), compared kernel by kernel:
  python tools/isa_diff.py parent.s change.s [-v] [--skeleton]
Per kernel symbol: its code between the entry label and the end of the function, with the local label
numbers renumbered in order of appearance, and its .amdhsa_kernel descriptor.  Prints "same" or
"differs" per kernel and whether the rest of the file (everything but the __hip_cuid_ symbol) is
the same; -v adds the first differing line of a kernel.  Exit status 1 if anything differs.

--skeleton: a kernel whose code differs is compared again by its descriptor (registers, accumulator
offset, scratch, LDS) and its skeleton -- the matrix, LDS, global / buffer / flat memory, s_waitcnt
and s_barrier instructions in order, with their operands -- and is "skeleton same" when both agree:
the scalar and vector arithmetic between them may differ.  Exit status 1 only for "differs"."""
import re
import subprocess
import sys

SKELETON = re.compile(r"\s*(v_mfma|ds_|global_|buffer_|flat_|s_waitcnt|s_barrier\b)")


def kernels(text):
  """name -> (code lines, descriptor lines)"""
  out = {}
  for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
    name, desc = m.group(1), m.group(2)
    body = re.search(r"^" + re.escape(name) + r":.*?^\.Lfunc_end\d+:", text, re.S | re.M)
    labels = {}
    def renumber(l):
      return labels.setdefault(l.group(0), ".L%d" % len(labels))
    code = re.sub(r"\.L(?:BB|func_end|tmp)\d+(?:_\d+)?", renumber, body.group(0) if body else "")
    out[name] = (code.splitlines(), desc.splitlines())
  return out


def skeleton(code):
  return [l.split(";")[0].strip() for l in code if SKELETON.match(l)]


def rest(text):
  return [l for l in text.splitlines() if "__hip_cuid_" not in l]


def first_difference(a, b):
  i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
  return "%d / %d lines, first difference at %d:\n    < %s\n    > %s" % (
      len(a), len(b), i, a[i] if i < len(a) else "", b[i] if i < len(b) else "")


def main():
  flags = {"-v", "--skeleton"}
  verbose, skel = "-v" in sys.argv, "--skeleton" in sys.argv
  pa, pb = [a for a in sys.argv[1:] if a not in flags]
  ta, tb = open(pa).read(), open(pb).read()
  ka, kb = kernels(ta), kernels(tb)
  count = {}
  for name in sorted(set(ka) | set(kb)):
    detail = None
    if name not in ka or name not in kb:
      verdict = "only in " + (pa if name in ka else pb)
    else:
      (ca, da), (cb, db) = ka[name], kb[name]
      if ca + da == cb + db:
        verdict = "same"
      elif skel and da == db and skeleton(ca) == skeleton(cb):
        verdict, detail = "skeleton same", first_difference(ca, cb)
      elif skel and da != db:
        verdict, detail = "differs", "descriptor: " + first_difference(da, db)
      elif skel:
        verdict, detail = "differs", "skeleton: " + first_difference(skeleton(ca), skeleton(cb))
      else:
        verdict, detail = "differs", first_difference(ca + da, cb + db)
    count[verdict] = count.get(verdict, 0) + 1
    dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    print("%-*s %s" % (13 if skel else 8, verdict, re.sub(r"\(.*", "", dn).replace("snnqp::", "").replace("void ", "")))
    if verbose and detail:
      print("    " + detail)
  whole = rest(ta) == rest(tb)
  total = len(set(ka) | set(kb))
  bad = total - count.get("same", 0) - count.get("skeleton same", 0)
  if skel:
    print("%d kernels, %d same, %d skeleton same, %d differ; whole file %s" % (
        total, count.get("same", 0), count.get("skeleton same", 0), bad, "same" if whole else "differs"))
    sys.exit(0 if bad == 0 else 1)
  print("%d kernels, %d not the same; whole file %s" % (total, bad, "same" if whole else "differs"))
  sys.exit(0 if bad == 0 and (whole or ka) else 1)


if __name__ == "__main__":
  main()
