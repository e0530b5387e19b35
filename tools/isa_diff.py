"""Two device-only assembly files (hipcc ... --cuda-device-only -S, as tools/kernel_regs.py compiles
them), compared kernel by kernel:
  python tools/isa_diff.py parent.s change.s [-v]
Per kernel symbol: its code between the entry label and the end of the function, with the local label
numbers renumbered in order of appearance, and its .amdhsa_kernel descriptor.  Prints "same" or
"differs" per kernel and whether the rest of the file (everything but the __hip_cuid_ symbol) is
the same; -v adds the first differing line of a kernel.  Exit status 1 if anything differs."""
import re
import subprocess
import sys


def kernels(text):
  out = {}
  for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
    name, desc = m.group(1), m.group(2)
    body = re.search(r"^" + re.escape(name) + r":.*?^\.Lfunc_end\d+:", text, re.S | re.M)
    labels = {}
    def renumber(l):
      return labels.setdefault(l.group(0), ".L%d" % len(labels))
    code = re.sub(r"\.L(?:BB|func_end|tmp)\d+(?:_\d+)?", renumber, body.group(0) if body else "")
    out[name] = code.splitlines() + desc.splitlines()
  return out


def rest(text):
  return [l for l in text.splitlines() if "__hip_cuid_" not in l]


def main():
  verbose = "-v" in sys.argv
  pa, pb = [a for a in sys.argv[1:] if a != "-v"]
  ta, tb = open(pa).read(), open(pb).read()
  ka, kb = kernels(ta), kernels(tb)
  bad = 0
  for name in sorted(set(ka) | set(kb)):
    if name not in ka or name not in kb:
      verdict = "only in " + (pa if name in ka else pb)
    else:
      verdict = "same" if ka[name] == kb[name] else "differs"
    bad += verdict != "same"
    dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    print("%-8s %s" % (verdict, re.sub(r"\(.*", "", dn).replace("snnqp::", "").replace("void ", "")))
    if verbose and verdict == "differs":
      a, b = ka[name], kb[name]
      i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
      print("    %d / %d lines, first difference at %d:\n    < %s\n    > %s" % (
          len(a), len(b), i, a[i] if i < len(a) else "", b[i] if i < len(b) else ""))
  whole = rest(ta) == rest(tb)
  print("%d kernels, %d not the same; whole file %s" % (len(set(ka) | set(kb)), bad,
                                                        "same" if whole else "differs"))
  sys.exit(0 if bad == 0 and (whole or ka) else 1)


if __name__ == "__main__":
  main()
