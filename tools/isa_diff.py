#!/usr/bin/env python3
"""Did a source change move the device code?  python tools/isa_diff.py OLD.s NEW.s compares two gfx950 assembly files kernel by kernel.

The files are what tests/test_host_cpu.py::_device_assembly compiles: hipcc + build.HIPCC_FLAGS + build.TU_FLAGS[src] + -S
--cuda-device-only, one per .hip entry of build.LIB_SOURCES (python -c "from adanerf_amd import build; print(build.LIB_SOURCES)").

Per kernel the text from its .globl line to .end_amdhsa_kernel (the kernel descriptor included) is normalised: comments (from `;`) and
empty lines go, and every .L label is renamed to its order of first appearance inside the kernel (labels carry a function ordinal that
shifts when a kernel disappears).  Non-kernel symbols (__hip_cuid_*) are ignored, and a trailing `bool` template argument of
sample_mlp16x3_gen_kernel (removed with its `false` half) is dropped from the name.  Then every kernel present in both files is

  class I  identical: the normalised text is equal;
  class R  registers only: equal number of lines, equal mnemonic on every line, equal .amdhsa_* lines (registers, LDS, scratch,
           occupancy inputs), equal label structure -- the only differences are register numbers in operands;
  FAIL     anything else; the first differing line is printed.

Exit status 1 on any FAIL."""
import re
import subprocess
import sys

_LABEL = re.compile(r"\.L\w+")
_REG = re.compile(r"\b[vsa]\d+\b|\b[vsa]\[\d+:\d+\]")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path):
    """{demangled kernel name: normalised lines}"""
    text = open(path).read()
    raw = {}
    for chunk in re.split(r"\n\s*\.globl\s+", text)[1:]:
        name = chunk.split("\n", 1)[0].strip()
        if ".end_amdhsa_kernel" not in chunk:      # not a kernel (__hip_cuid_*, device variables)
            continue
        body = chunk.split(".end_amdhsa_kernel")[0] + ".end_amdhsa_kernel"
        lines = [ln.split(";")[0].strip() for ln in body.split("\n")]
        lines = [re.sub(r"\s+", " ", ln) for ln in lines if ln]
        raw[name] = lines
    pretty = demangle(sorted(raw))
    out = {}
    for name, lines in raw.items():
        shown = re.sub(r"(sample_mlp16x3_gen_kernel<[^>]*), (?:true|false)>", r"\1>", pretty[name])
        labels = {}
        txt = "\n".join(lines).replace(name, "<kernel>")      # the symbol itself: its mangling changes with the template arguments
        for m in _LABEL.finditer(txt):
            labels.setdefault(m.group(0), ".L%d" % len(labels))
        out[shown] = _LABEL.sub(lambda m: labels[m.group(0)], txt).split("\n")
    return out


def classify(a, b):
    """('I' | 'R' | 'FAIL', differing lines, first differing (index, old, new))"""
    if a == b:
        return "I", 0, None
    first = next(((i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y), (min(len(a), len(b)), "<end>", "<end>"))
    if len(a) != len(b):
        return "FAIL", abs(len(a) - len(b)), first
    n = 0
    for i, (x, y) in enumerate(zip(a, b)):
        if x == y:
            continue
        n += 1
        # same mnemonic, same labels, same immediates: equal once every register operand is blanked; descriptor lines must be equal
        if x.startswith(".amdhsa_") or x.split(" ", 1)[0] != y.split(" ", 1)[0] or _REG.sub("r", x) != _REG.sub("r", y):
            return "FAIL", n, (i, x, y)
    return "R", n, first


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    old, new = kernels(argv[1]), kernels(argv[2])
    print("OLD %s: %d kernels   NEW %s: %d kernels" % (argv[1], len(old), argv[2], len(new)))
    for title, names in (("only in OLD", sorted(set(old) - set(new))), ("only in NEW", sorted(set(new) - set(old)))):
        print("%s: %d" % (title, len(names)))
        for n in names:
            print("    " + n)
    res = {n: classify(old[n], new[n]) for n in sorted(set(old) & set(new))}
    count = {c: sum(1 for r in res.values() if r[0] == c) for c in ("I", "R", "FAIL")}
    print("class I (identical): %d   class R (registers only): %d   FAIL: %d" % (count["I"], count["R"], count["FAIL"]))
    for n, (c, lines, first) in res.items():
        if c == "R":
            print("  R    %s: %d of %d lines differ" % (n, lines, len(old[n])))
    for n, (c, lines, first) in res.items():
        if c == "FAIL":
            print("  FAIL %s (%d -> %d lines): first difference at line %d\n         old: %s\n         new: %s" %
                  (n, len(old[n]), len(new[n]), first[0], first[1], first[2]))
    return 1 if count["FAIL"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
