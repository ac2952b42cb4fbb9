"""Compare two device-assembly listings of one source file, kernel by kernel.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -mcode-object-version=5 \
        -I epfl_megatron_amd/csrc -S --cuda-device-only FILE.hip -o FILE.s   (both trees)
    python scripts/isa_compare.py BEFORE.s AFTER.s [--stream NAME_PART ...]

Every kernel is paired with the kernel of the same mangled name.  Without
--stream a kernel must be identical instruction for instruction (block-label
numbers erased).  A kernel whose name contains one of the --stream parts is a
persistent K-step kernel whose register allocation may move: for it the
script compares the resource metadata, the multiset of opcodes, and the
instruction sequence with register numbers erased, and says in which region
of the kernel every difference of that sequence lies:
    prologue | first-step (the tile loop up to the K-step loop) |
    k-loop (the innermost loop: the steady K-step) | epilogue (the rest of the
    tile loop) | tail
The regions come from the backward branches of the listing (an instruction
whose label operand is defined above it closes a loop); no instruction is
looked for by name.  Exit status 1 if any kernel fails its rule.
"""
import argparse
import collections
import difflib
import re
import sys

META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
             "private_segment_fixed_size", "group_segment_fixed_size")
LABEL = re.compile(r"\.LBB\d+_\d+")
REG_RANGE = re.compile(r"\b([vsa])\[(\d+):(\d+)\]")
REG = re.compile(r"\b([vsa])\d+\b")


def parse(path):
    """-> ({kernel: [(label or None, instruction text)]}, {kernel: metadata})"""
    kernels, meta, cur, entry = {}, {}, None, None
    pending = None
    for line in open(path):
        code = line.split(";", 1)[0].rstrip()
        if cur is None:
            m = re.match(r"\s+\.type\s+(\S+),@function", code)
            if m:
                cur = m.group(1)
                kernels[cur] = []
                continue
            m = re.match(r"  - \.(\w+):\s+(\S+)", code)
            if m:
                entry = {m.group(1): m.group(2)}
                continue
            m = re.match(r"    \.(\w+):\s+(\S+)", code)
            if m and entry is not None:
                entry[m.group(1)] = m.group(2)
                if m.group(1) == "name":
                    meta[m.group(2)] = entry
            continue
        s = code.strip()
        if s.startswith(".Lfunc_end"):
            cur, pending = None, None
        elif s.endswith(":"):
            if LABEL.fullmatch(s[:-1]):
                pending = s[:-1]
        elif s and not s.startswith("."):
            kernels[cur].append((pending, " ".join(s.split())))
            pending = None
    return kernels, meta


def no_labels(ins):
    return [LABEL.sub(".LBB", t) for _, t in ins]


def no_regs(ins):
    out = []
    for t in no_labels(ins):
        t = REG_RANGE.sub(lambda m: f"{m.group(1)}[#{int(m.group(3)) - int(m.group(2)) + 1}]", t)
        out.append(REG.sub(lambda m: m.group(1) + "#", t))
    return out


def loops(ins):
    """[(head index, closing branch index)] of the backward branches"""
    at, out = {}, []
    for i, (lab, t) in enumerate(ins):
        if lab:
            at[lab] = i
        m = LABEL.search(t)
        if m and m.group(0) in at:
            out.append((at[m.group(0)], i))
    return out


def regions(ins):
    """index -> region name, from the outermost and the largest innermost loop"""
    lp = loops(ins)
    if not lp:
        return lambda i: "whole"
    outer = max(lp, key=lambda l: l[1] - l[0])
    inner = [l for l in lp if l != outer and outer[0] <= l[0] and l[1] <= outer[1]]
    inner = [l for l in inner if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in inner)]
    k = max(inner, key=lambda l: l[1] - l[0]) if inner else outer

    def name(i):
        if k[0] <= i <= k[1]:
            return "k-loop"
        if i < outer[0]:
            return "prologue"
        if i > outer[1]:
            return "tail"
        return "first-step" if i < k[0] else "epilogue"
    return name


def compare_stream(name, a, b, ma, mb):
    ok = True
    lines = []
    bad = [k for k in META_KEYS if ma.get(k) != mb.get(k)]
    ok &= not bad
    lines.append("  metadata " + ("same: " if not bad else "DIFFERS: ") +
                 " ".join(f"{k}={ma.get(k)}" + ("" if ma.get(k) == mb.get(k) else f"->{mb.get(k)}")
                          for k in META_KEYS))
    oa = collections.Counter(t.split()[0] for _, t in a)
    ob = collections.Counter(t.split()[0] for _, t in b)
    ok &= oa == ob
    lines.append(f"  opcode multiset {'same' if oa == ob else 'DIFFERS: ' + str((oa - ob) + (ob - oa))}"
                 f" ({len(a)} -> {len(b)} instructions)")
    na, nb = no_regs(a), no_regs(b)
    ra, rb = regions(a), regions(b)
    where = collections.Counter()
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, na, nb, autojunk=False).get_opcodes():
        if tag == "equal":
            continue
        for i in range(i1, i2):
            where[ra(i)] += 1
        for j in range(j1, j2):
            where[rb(j)] += 1
    ka = [t for i, t in enumerate(na) if ra(i) == "k-loop"]
    kb = [t for j, t in enumerate(nb) if rb(j) == "k-loop"]
    ok &= ka == kb
    lines.append(f"  k-loop sequence (registers erased) {'same' if ka == kb else 'DIFFERS'}"
                 f" ({len(ka)} instructions)")
    if where:
        lines.append("  differing positions by region: " +
                     " ".join(f"{r}={n}" for r, n in sorted(where.items())))
    else:
        lines.append("  whole sequence (registers erased) same")
    return ok, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--stream", nargs="*", default=[], help="name parts of the K-step kernels")
    args = ap.parse_args()
    ka, ma = parse(args.before)
    kb, mb = parse(args.after)
    allok = True
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            print(f"{name}\n  only in {'before' if name in ka else 'after'}")
            continue
        if any(s in name for s in args.stream):
            ok, lines = compare_stream(name, ka[name], kb[name], ma.get(name, {}), mb.get(name, {}))
        else:
            ok = no_labels(ka[name]) == no_labels(kb[name])
            lines = [f"  {'identical' if ok else 'DIFFERS'} ({len(ka[name])} -> {len(kb[name])} instructions)"]
        allok &= ok
        print(f"{name}  {'ok' if ok else 'FAIL'}")
        print("\n".join(lines))
    print("ALL OK" if allok else "SOME KERNELS FAIL")
    return 0 if allok else 1


if __name__ == "__main__":
    sys.exit(main())
