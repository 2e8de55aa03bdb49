#!/usr/bin/env python3
"""Development helper: compare every kernel of two `hipcc --cuda-device-only -S` files (parent build, new build) - what a
refactor that must not move the code has to show.
    python tools/isa_compare.py parent/encode.s new/encode.s [--loop-blocks] [--map PARENT_NAME_PART=NEW_NAME_PART ...]
--map: a renamed kernel is compared with the parent instance it replaces - the parent's (mangled) kernel names go through
re.sub(PARENT_NAME_PART, NEW_NAME_PART) before the two sides are matched, e.g.
    --map '22pq_store_ragged_kernelILi(.)EEEvNS_17StoreRaggedParamsE=18paged_store_kernelILi\\1ENS_17StoreRaggedParamsEEEvT0_'
Per kernel: VGPR / AGPR / SGPR counts, static LDS, scratch, spills, code length, the opcode histogram, and the largest basic
block by text length, picked as tools/isa_count.py picks it, with its vector-ALU count (columns big / big_valu).  That block
is the unrolled centroid loop where the loop is one block; where the unrolled loop is split into several blocks (d_m = 1
through the scalar cache, the LDS kernels) it is merely the longest block - still the same block on both sides.  The histogram may differ in padding, waits,
moves and branches (ALLOWED) only, and so may the largest block; everything else must be equal.  --loop-blocks adds, per kernel, the
basic blocks that hold an MFMA and a global load and no LDS write (the unrolled code-tile loop of the decode kernels; the blocks of their
residual-window pass fill an LDS tile), compared in order: their histograms may differ by ALLOWED and by how LDS reads of the same total
width are grouped; "LOOP MISS" otherwise (counted as a miss); and it says under every kernel where its other differences sit: in
front of its first MFMA, between its first and last MFMA (the tile loops with their set-up), behind its last MFMA (the tail).  Opcodes are counted without their encoding suffix (_e32,
_e64, _sdwa, _dpp): the same compare in another encoding is the same instruction.  Exit status 1 if any kernel misses that."""
import collections
import re
import sys

ALLOWED = ("s_nop", "s_waitcnt", "s_mov_b32", "v_mov_b32", "s_branch", "s_cbranch")
FIG = [("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"),
       ("scratch", r"; ScratchSize: (\d+)"), ("len", r"; codeLenInByte = (\d+)")]


ENC = re.compile(r"_(e32|e64|sdwa|dpp)$")


def kernels(path, renames=()):
    s = open(path).read()
    spills = {m.group(1): (m.group(2), m.group(3)) for m in
              re.finditer(r"\.name:\s+(_Z\w+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", s)}
    out = {}
    for name in re.findall(r"^(_Z\w+):\s*(?:;.*)?$", s, re.M):
        tail = s[s.index(name + ":"):]
        end = re.search(r"^\.Lfunc_end\d+:", tail, re.M)
        if not end:
            continue
        body = tail[:end.start()]
        ops = lambda text: collections.Counter(ENC.sub("", l.split()[0]) for l in text.splitlines()[1:] if l.strip() and not l.strip().startswith((".", ";")) and not l.strip().endswith(":"))
        blocks = re.split(r"^\.LBB\d+_\d+:.*$", body, flags=re.M)
        big = ops(max(blocks, key=len))
        loops = [ops(bl) for bl in blocks if "v_mfma" in bl and "global_load" in bl and "ds_write" not in bl]
        fig = {k: re.search(rx, tail).group(1) for k, rx in FIG}
        fig["sgpr_spill"], fig["vgpr_spill"] = spills.get(name, ("?", "?"))
        fig["big"] = str(sum(big.values()))
        fig["big_valu"] = str(sum(v for k, v in big.items() if k.startswith("v_")))
        text = [re.sub(r"\s*;.*$", "", l).strip() for l in body.splitlines()[1:]]
        for old, new in renames:
            name = re.sub(old, new, name)
        seq = [ENC.sub("", l.split()[0]) for l in text if l and not l.startswith((".", ";")) and not l.endswith(":")]
        mf = [i for i, o in enumerate(seq) if o.startswith("v_mfma")] or [len(seq), len(seq) - 1]
        parts = [collections.Counter(p) for p in (seq[:mf[0]], seq[mf[0]:mf[-1] + 1], seq[mf[-1] + 1:])]
        out[name] = (fig, ops(body), [l for l in text if l], big, loops, parts)
    return out


DS_BITS = re.compile(r"ds_read(2|2st64)?_[bu](\d+)")


def loop_key(h):
    """A block's histogram without ALLOWED, its LDS reads as one total width."""
    k = {op: n for op, n in h.items() if not op.startswith(ALLOWED) and not DS_BITS.match(op)}
    k["ds_read bits"] = sum(n * int(m.group(2)) * (2 if m.group(1) else 1) for op, n in h.items() for m in [DS_BITS.match(op)] if m)
    return k


args = sys.argv[1:]
loop_blocks = "--loop-blocks" in args
if loop_blocks:
    args.remove("--loop-blocks")
renames = []
while "--map" in args:
    i = args.index("--map")
    renames.append(tuple(args[i + 1].split("=", 1)))
    del args[i:i + 2]
sys.argv[1:] = args
a, b = kernels(sys.argv[1], renames), kernels(sys.argv[2])
bad = 0
cols = [k for k, _ in FIG] + ["sgpr_spill", "vgpr_spill", "big", "big_valu"]
print(f"{sys.argv[1]} (parent) | {sys.argv[2]} (new); {len(a)} / {len(b)} kernels")
print("kernel: " + " ".join(cols) + "  [parent | new]  verdict")
for name in sorted(set(a) | set(b)):
    if name not in a or name not in b:
        print(f"{name}: only in {'parent' if name in a else 'new'}  MISS")
        bad += 1
        continue
    (fa, ha, ta, ba, la, pa), (fb, hb, tb, bb, lb, pb) = a[name], b[name]
    diff = {k: (ha[k], hb[k]) for k in set(ha) | set(hb) if ha[k] != hb[k]}
    hard = {k: v for k, v in diff.items() if not k.startswith(ALLOWED)}
    # the largest block may differ by the allowed opcodes only
    big_ok = all(k.startswith(ALLOWED) for k in set(ba) | set(bb) if ba[k] != bb[k])
    figs_ok = all(fa[k] == fb[k] for k in cols if k not in ("len", "big", "big_valu")) and big_ok
    verdict = "text identical" if ta == tb else "text differs" + (f", histogram differs in {dict(sorted(diff.items()))}" if diff else ", histogram equal")
    if hard or not figs_ok:
        verdict += "  MISS"
        bad += 1
    if loop_blocks:
        same = len(la) == len(lb) and all(loop_key(x) == loop_key(y) for x, y in zip(la, lb))
        verdict += f"; loop blocks {len(la)} | {len(lb)}, sizes {[sum(x.values()) for x in la]} | {[sum(x.values()) for x in lb]}" + ("" if same else "  LOOP MISS")
        if not same and not (hard or not figs_ok):
            bad += 1
    print(f"{name}: {' '.join(fa[k] for k in cols)} | {' '.join(fb[k] for k in cols)}  {verdict}")
    for part, x, y in zip(("front", "tile loops", "tail"), pa, pb) if loop_blocks and ta != tb else ():
        d = [f"{k} {x[k]}->{y[k]}" for k in sorted(set(x) | set(y)) if x[k] != y[k] and not k.startswith(ALLOWED)]
        print(f"    {part}: {sum(x.values())} | {sum(y.values())} instructions; " + (", ".join(d) or "equal but for the allowed opcodes"))
print(f"{bad} kernel(s) miss the rule" if bad else "every kernel meets the rule")
sys.exit(1 if bad else 0)
