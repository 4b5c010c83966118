#!/usr/bin/env python
"""Are two device assembly files the same code, kernel by kernel?  The check of a refactor that must not move the ISA.

    hipcc <build.py's FLAGS> --cuda-device-only -S old/x.hip -o old.s      (and the same for the new tree)
    python tools/isa_same.py old.s new.s [-o table.json]

Per kernel symbol (every `.amdhsa_kernel` of either file): the instruction stream -- comments and directives dropped,
`.LBB` labels renumbered by first appearance -- and .vgpr_count, .sgpr_count, .private_segment_fixed_size,
.group_segment_fixed_size, .kernarg_segment_size of the metadata.  Prints one row per kernel; exit status 1 on any
difference or on a kernel that only one side has.  Host only, no GPU.
"""
import json
import re
import sys

FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
          "kernarg_segment_size")


def kernels(path):
    """{symbol: (instructions, {field: value})}"""
    lines = open(path).read().split("\n")
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    streams, cur, labels = {}, None, {}
    for raw in lines:
        line = raw.split(";")[0].strip()
        if cur is None:
            if line.endswith(":") and line[:-1] in names:
                cur, labels = line[:-1], {}
                streams[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        elif line and (not line.startswith(".") or line.endswith(":")):      # an instruction or a label
            streams[cur].append(re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)),
                                       " ".join(line.split())))
    meta = {}
    for entry in re.split(r"^  - (?=\.)", "\n".join(lines).split(".amdgpu_metadata")[1], flags=re.M)[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", entry, re.M).group(1)
        meta[name] = {f: int(re.search(r"^\s*\.%s:\s+(\d+)" % f, entry, re.M).group(1)) for f in FIELDS}
    return {k: (streams.get(k, []), meta.get(k, {})) for k in names}


def main():
    args = [x for x in sys.argv[1:] if x != "-o"]
    out = args.pop(sys.argv.index("-o") - 1) if "-o" in sys.argv else None
    old, new = kernels(args[0]), kernels(args[1])
    rows, same_all = [], True
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            rows.append([k, None, None, None, None, "only in " + (args[0] if k in old else args[1])])
            same_all = False
            continue
        (io, mo), (ix, mx) = old[k], new[k]
        what = [] if io == ix else ["instructions"]
        what += [f for f in FIELDS if mo.get(f) != mx.get(f)]
        if not io:
            what.append("no instructions found")
        same_all = same_all and not what
        rows.append([k, len(ix), mx.get("vgpr_count"), mx.get("sgpr_count"), mx.get("private_segment_fixed_size"),
                     "yes" if not what else "NO: " + ", ".join(what)])
    print("%-90s %8s %5s %5s %8s  %s" % ("kernel", "instr", "vgpr", "sgpr", "scratch", "identical"))
    for r in rows:
        print("%-90s %8s %5s %5s %8s  %s" % tuple(r))
    print("%d kernels, %s" % (len(rows), "all identical" if same_all else "DIFFERENCES"))
    if out:
        with open(out, "w") as fh:
            json.dump({"kernels": len(rows), "all_identical": same_all,
                       "columns": ["kernel", "instructions", "vgpr", "sgpr", "scratch", "identical"], "table": rows},
                      fh, indent=1)
    return 0 if same_all else 1


if __name__ == "__main__":
    sys.exit(main())
