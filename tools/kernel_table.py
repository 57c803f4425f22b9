#!/usr/bin/env python3
"""Side-by-side code-object table of two builds' kernels, from the gfx950 assembly `hipcc -save-temps` leaves behind.

    tools/kernel_table.py PARENT_DIR PR_DIR > profiles/frame_split_kernels.txt

Each directory holds the `*-hip-amdgcn-amd-amdhsa-gfx950.s` files of one build.  Per kernel: VGPRs, SGPRs, both spill counts,
scratch bytes, static LDS bytes and the number of instructions on each side, and whether the instruction text is the same once
basic-block labels are renumbered in order of appearance."""
import glob
import re
import sys


def functions(path):
    """{function name: [instruction lines]} and {kernel name: metadata dict} of one assembly file."""
    text = open(path).read()
    body, meta = {}, {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        lines = []
        for ln in m.group(2).split("\n"):
            ln = ln.split(";")[0].rstrip()
            if not ln.strip() or (ln.strip().startswith(".") and not ln.strip().startswith(".LBB")):
                continue
            lines.append(ln.strip())
        body[m.group(1)] = lines
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target)", text, re.S | re.M):
        d = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)$", m.group(0), re.M))
        meta[d["name"]] = d
    return body, meta


def short(name):
    m = re.match(r"_Z(\d+)", name)
    return name[m.end():m.end() + int(m.group(1))] if m else name


def normalised(lines):
    labels = {}
    def ren(m):
        return labels.setdefault(m.group(0), ".L%d" % len(labels))
    return [re.sub(r"\.LBB\d+_\d+", ren, ln) for ln in lines]


def load(d):
    body, meta = {}, {}
    for p in sorted(glob.glob(d + "/*gfx950.s")):
        b, m = functions(p)
        body.update({short(k): v for k, v in b.items()})
        meta.update({short(k): v for k, v in m.items()})
    return body, meta


def main():
    (pb, pm), (nb, nm) = load(sys.argv[1]), load(sys.argv[2])
    cols = [("vgpr_count", "VGPR"), ("sgpr_count", "SGPR"), ("vgpr_spill_count", "vspill"), ("sgpr_spill_count", "sspill"),
            ("private_segment_fixed_size", "scratch"), ("group_segment_fixed_size", "LDS")]
    print("%-30s %s %11s  %s" % ("kernel (parent / this tree)", " ".join("%11s" % c[1] for c in cols), "instr", "text"))
    differ = 0
    for k in sorted(set(pm) | set(nm)):
        cells = ["%5s/%-5s" % (pm.get(k, {}).get(c, "-"), nm.get(k, {}).get(c, "-")) for c, _ in cols]
        ni = "%5d/%-5d" % (len(pb.get(k, [])), len(nb.get(k, [])))
        same = normalised(pb.get(k, [])) == normalised(nb.get(k, [None]))
        differ += not same
        print("%-30s %s %11s  %s" % (k, " ".join(cells), ni, "same" if same else "DIFFERS"))
    print("\ndevice functions called from them (not inlined):")
    for k in sorted((set(pb) | set(nb)) - set(pm) - set(nm)):
        same = normalised(pb.get(k, [])) == normalised(nb.get(k, [None]))
        differ += not same
        print("%-30s %83s  %s" % (k, "%5d/%-5d" % (len(pb.get(k, [])), len(nb.get(k, []))), "same" if same else "DIFFERS"))
    print("\n%d of %d differ" % (differ, len(set(pb) | set(nb))))


if __name__ == "__main__":
    main()
