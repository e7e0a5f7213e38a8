#!/usr/bin/env python3
"""kernel_text_diff.py PARENT.s NEW.s -- compare the device code of two builds of one
translation unit, kernel by kernel.

Both files are hipcc's device assembly of the same source at two commits, built with the
Makefile's CXXFLAGS plus `--cuda-device-only -S`.  Directive and comment lines are dropped;
every kernel (amdhsa kernel symbol) is then put into one class:

  identical      the instruction text is the same, line for line;
  labels only    the same once the numbers of local labels are masked (.LBB<f>_<n> carries the
                 function's index in the file, which moves when a function before it comes or
                 goes);
  prologue only  the texts differ only before the kernel's first s_barrier and are equal after
                 it once register numbers and local labels are masked;
  body changed   anything else (a kernel without an s_barrier that differs lands here);
  only in ...    the symbol exists on one side only.

Per kernel it also prints .vgpr_count, .sgpr_count, scratch (.private_segment_fixed_size), LDS
(.group_segment_fixed_size) and the code length in bytes of both sides.  Exit status 0 when
every kernel is identical, 1 otherwise."""
import re
import shutil
import subprocess
import sys

REG = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(_\d+)?")


def parse(path):
    """{kernel symbol: (instruction lines, {metadata})}"""
    text = open(path).read().split("\n")
    kernels = {l.split()[1] for l in text if l.strip().startswith(".amdhsa_kernel ")}
    body, meta = {}, {}
    cur = None
    for l in text:
        s = l.strip()
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if m and m.group(1) in kernels and cur is None and m.group(1) not in body:
            cur = m.group(1)
            body[cur] = []
            meta[cur] = {}
            continue
        if cur is None:
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if not s or s.startswith(";"):
            continue
        if s.startswith(".") and not s.endswith(":"):
            continue  # directive (local labels end with ':')
        body[cur].append(s.split(";")[0].rstrip())
    # code length: the "; codeLenInByte = N" comment behind each function, in file order
    order = [l.split(":")[0] for l in text if re.match(r"^[A-Za-z_][\w$.]*:", l) and l.split(":")[0] in kernels]
    lens = [int(m.group(1)) for m in re.finditer(r"; codeLenInByte = (\d+)", "\n".join(text))]
    funcs = [l.split(":")[0] for l in text if re.match(r"^[A-Za-z_][\w$.]*:\s*(;.*)?$", l) and not l.startswith(".")]
    if len(lens) == len(funcs):
        for f, n in zip(funcs, lens):
            if f in meta:
                meta[f]["code"] = n
    elif len(lens) == len(order):
        for f, n in zip(order, lens):
            meta[f]["code"] = n
    # amdgpu metadata (YAML): entries keyed by .name
    ent = {}
    for l in text:
        s = l.strip()
        if s.startswith("- .") or s.startswith("-   ."):
            s = s.lstrip("- ")
        m = re.match(r"^\.(\w+):\s*(\S+)$", s)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size",
                 "group_segment_fixed_size", "agpr_count"):
            ent[k] = v
        elif k == "name":
            ent["name"] = v
        elif k == "wavefront_size":  # the last key of a kernel entry (keys are sorted)
            if ent.get("name") in meta:
                meta[ent["name"]].update({a: b for a, b in ent.items() if a != "name"})
            ent = {}
    return body, meta


def mask(line):
    return LABEL.sub(".L", REG.sub(lambda m: m.group(1) + ("[]" if m.group(2)[0] == "[" else "#"), line))


def first_barrier(lines):
    for i, l in enumerate(lines):
        if l.startswith("s_barrier"):
            return i
    return -1


def classify(a, b):
    if a == b:
        return "identical"
    if [LABEL.sub(".L", l) for l in a] == [LABEL.sub(".L", l) for l in b]:
        return "labels only"
    ia, ib = first_barrier(a), first_barrier(b)
    if ia >= 0 and ib >= 0 and [mask(l) for l in a[ia:]] == [mask(l) for l in b[ib:]]:
        return "prologue only"
    return "body changed"


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool] + list(names), capture_output=True, text=True).stdout.split("\n")
    return {n: (o if o else n) for n, o in zip(names, out)}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (ba, ma), (bb, mb) = parse(sys.argv[1]), parse(sys.argv[2])
    names = sorted(set(ba) | set(bb))
    pretty = demangle(names)
    keys = (("vgpr_count", "vgpr"), ("sgpr_count", "sgpr"), ("private_segment_fixed_size", "scratch"),
            ("group_segment_fixed_size", "lds"), ("code", "code"))
    worst = 0
    for n in names:
        if n not in ba or n not in bb:
            cls = "only in " + ("parent" if n in ba else "new")
        else:
            cls = classify(ba[n], bb[n])
        worst |= cls != "identical"
        figs = "  ".join(f"{short} {ma.get(n, {}).get(k, '-')}/{mb.get(n, {}).get(k, '-')}" for k, short in keys)
        print(f"{cls:14s} {pretty[n]}\n{'':14s} {figs}  (parent/new)")
    return int(worst)


if __name__ == "__main__":
    sys.exit(main())
