#!/usr/bin/env python3
"""Development helper: compare every kernel of two `hipcc --cuda-device-only -S` files (parent build, new build) - what a
refactor that must not move the code has to show.
    python tools/isa_compare.py parent/encode.s new/encode.s
Per kernel: VGPR / AGPR / SGPR counts, static LDS, scratch, spills, code length, the opcode histogram, and the largest basic
block by text length, picked as tools/isa_count.py picks it, with its vector-ALU count (columns big / big_valu).  That block
is the unrolled centroid loop where the loop is one block; where the unrolled loop is split into several blocks (d_m = 1
through the scalar cache, the LDS kernels) it is merely the longest block - still the same block on both sides.  The histogram may differ in padding, waits,
moves and branches (ALLOWED) only; everything else must be equal.  Exit status 1 if any kernel misses that."""
import collections
import re
import sys

ALLOWED = ("s_nop", "s_waitcnt", "s_mov_b32", "v_mov_b32", "s_branch", "s_cbranch")
FIG = [("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"),
       ("scratch", r"; ScratchSize: (\d+)"), ("len", r"; codeLenInByte = (\d+)")]


def kernels(path):
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
        ops = lambda text: collections.Counter(l.split()[0] for l in text.splitlines()[1:] if l.strip() and not l.strip().startswith((".", ";")) and not l.strip().endswith(":"))
        big = ops(max(re.split(r"^\.LBB\d+_\d+:.*$", body, flags=re.M), key=len))
        fig = {k: re.search(rx, tail).group(1) for k, rx in FIG}
        fig["sgpr_spill"], fig["vgpr_spill"] = spills.get(name, ("?", "?"))
        fig["big"] = str(sum(big.values()))
        fig["big_valu"] = str(sum(v for k, v in big.items() if k.startswith("v_")))
        text = [re.sub(r"\s*;.*$", "", l).strip() for l in body.splitlines()[1:]]
        out[name] = (fig, ops(body), [l for l in text if l])
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
bad = 0
cols = [k for k, _ in FIG] + ["sgpr_spill", "vgpr_spill", "big", "big_valu"]
print(f"{sys.argv[1]} (parent) | {sys.argv[2]} (new); {len(a)} / {len(b)} kernels")
print("kernel: " + " ".join(cols) + "  [parent | new]  verdict")
for name in sorted(set(a) | set(b)):
    if name not in a or name not in b:
        print(f"{name}: only in {'parent' if name in a else 'new'}  MISS")
        bad += 1
        continue
    (fa, ha, ta), (fb, hb, tb) = a[name], b[name]
    diff = {k: (ha[k], hb[k]) for k in set(ha) | set(hb) if ha[k] != hb[k]}
    hard = {k: v for k, v in diff.items() if not k.startswith(ALLOWED)}
    figs_ok = all(fa[k] == fb[k] for k in cols if k != "len")
    verdict = "text identical" if ta == tb else "text differs" + (f", histogram differs in {dict(sorted(diff.items()))}" if diff else ", histogram equal")
    if hard or not figs_ok:
        verdict += "  MISS"
        bad += 1
    print(f"{name}: {' '.join(fa[k] for k in cols)} | {' '.join(fb[k] for k in cols)}  {verdict}")
print(f"{bad} kernel(s) miss the rule" if bad else "every kernel meets the rule")
sys.exit(1 if bad else 0)
