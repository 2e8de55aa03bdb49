"""GPU tests of the decode-step attention - attn_lean_kernel, attn_stream_kernel and their split merge (csrc/attn_lean.h,
attn_stream.h, attn_tail.h), the tile and scalar kernels (csrc/attn_tile.hip, attn_generic.hip) - against the fp64 oracle, with
the project's bar of rel-L2 < 1e-3 applied to EVERY head (tests/decode_inputs.py: check_heads) on inputs shaped like attention in
a language model (tests/flash_inputs.py: logit spreads of 1 .. 8, outlier channels, a sink with a recency ramp, staircases that
move the lazy softmax reference in every unit, rows whose tail is fp16-subnormal, scaled V, one dominating key in the codes, the
window or the appended row).  Every call runs through decode_poison.run on the case's clean copy, under the case's policy, on
the kernel the case names; no split merge may give up.  tests/test_decode_numerics_host.py shows on the CPU that these inputs
leave a correct kernel half the bar of room, and that the many-pairs case catches flushed fp16-subnormal probabilities."""
import dataclasses

import numpy as np
import pytest

from tests import decode_inputs as D
from tests import decode_poison as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    return torch, ops, _lib.load(), _lib


def _run(env, c, built):
    """One call on the clean copy under c's policy: the kernel kind c names, no merge that gave up.  -> out (bs, nh, 1, d)"""
    torch, ops, lib, L = env
    got = P.kernel_kind(c, lib, L)
    assert got == c.kind, f"{c.name}: kernel kind {got}, expected {c.kind}"
    res = P.run(c, built["clean"], torch, ops, lib, L)
    faults = ops.tail_faults()
    assert faults == 0, f"{c.name}: {faults} split merges gave up"
    return res["out"]


def _case(env, oracle, c, name, src=None):
    src = D.for_case(name, c) if src is None else src
    built = P.build(c, src)
    out = _run(env, c, built)
    D.check_heads(out, P.gold(c, built, oracle), f"{c.name} {name}", name)
    return out, built


# ---------------------------------------------------------------- a. every family on one case per kernel form ------------
A_PAIRS = [(cn, n) for cn in D.SECTION_A for n in D.NAMES if D.has_peak(P.BY_NAME[cn], D.split_name(n)[1])]


@pytest.mark.parametrize("cname,name", A_PAIRS, ids=lambda x: x)
def test_decode_heads_on_llm_shaped_inputs(cname, name, env, oracle):
    """stair9 moves the lazy reference in every unit, stair5 in every second one; with sink_local on an appending case the highest
    local score arrives through the append path; a peak makes one wave's (or one split's) reference dwarf the others' in the merges."""
    _case(env, oracle, P.BY_NAME[cname], name)


# ---------------------------------------------------------------- b. every case of the matrix -----------------------------
B_PAIRS = [(c.name, n) for c in P.CASES for n in D.SECTION_B_NAMES if (c.name, n) not in A_PAIRS]


@pytest.mark.parametrize("cname,name", B_PAIRS, ids=lambda x: x)
def test_decode_heads_on_every_case_of_the_matrix(cname, name, env, oracle):
    """Every layout, id width and length mode of decode_poison.CASES under the per-head bar (the pairs of these two families
    that section a. runs are not run twice)."""
    _case(env, oracle, P.BY_NAME[cname], name)


# ---------------------------------------------------------------- c. many pairs, one split --------------------------------
@pytest.fixture(scope="module")
def many_pairs(env, oracle):
    """name -> (built, gold), built once (and one family at a time: 0.3 GB each)."""
    torch = env[0]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            c = D.many_pairs_case(0, cus)
            built = P.build(c, D.for_case(name, c))
            cache[name] = (built, P.gold(c, built, oracle))
        return cache[name] + (cus,)
    return get


@pytest.mark.parametrize("policy", [0, 16], ids=["lean", "stream"])
@pytest.mark.parametrize("name", D.MANY_PAIRS_NAMES)
def test_decode_heads_with_one_split_per_pair(name, policy, many_pairs, env):
    """bs = ceil(CUs / 8) requests x 8 kv heads at T = 4096: the split policy (about one workgroup per CU: ceil(CUs / pairs)
    splits) gives ONE split per (request, kv head) - the library does not report the count; it follows from bs * nh_k >= CUs
    and cap <= 128 - so a wave streams 512 keys under one lazy reference.  In `descending` key 0 is the maximum and the
    probabilities of the other keys of its wave are 2^-10 .. 2^-20 of it, partly fp16-subnormal: a value product that flushed
    them would miss the bar by 2 x on every head (test_decode_numerics_host.py).  Gold for every pair, through the C oracle."""
    built, gold, cus = many_pairs(name)
    c = D.many_pairs_case(policy, cus)
    assert c.bs * c.nhk >= cus and c.cap <= 128 and D.mfma_splits(c.T_host, c.bs * c.nhk, c.cap, cus) == 1
    D.check_heads(_run(env, c, built), gold, f"{c.name} one split {name} T{c.T} bs{c.bs}", name)


# ---------------------------------------------------------------- d. every head grouping ----------------------------------
@pytest.mark.parametrize("form", D.GROUP_FORMS, ids=[f[0] for f in D.GROUP_FORMS])
@pytest.mark.parametrize("G", D.GROUPINGS)
def test_decode_every_head_grouping(G, form, env, oracle):
    """Where heads differ between the kernels: the last, shorter part of 5 .. 16 heads run as virtual kv heads (d = 64, and
    d = 128 / M = 16), the second register row at 9 .. 16 heads (streaming kernel), the idle score columns >= G, and which
    workgroup merges which head.  gauss4, and a dominating key that only the last head of every group, or only head 0, sees."""
    c = D.group_case(*form, G)
    for name in D.GROUP_NAMES:
        _case(env, oracle, c, name, D.group_inputs(name, c))


# ---------------------------------------------------------------- e. lengths at the edges ---------------------------------
@pytest.mark.parametrize("policy", [0, 16], ids=["lean", "stream"])
def test_decode_ragged_lengths_at_unit_and_page_edges(policy, env, oracle):
    """One launch with device-resident lengths whose requests have T on both sides of the 32- and 64-token units, the 512-token
    split length and 1024, and r in {0, 1, 127, 128} at ring starts that wrap; the per-head bar for every request."""
    torch, ops, lib, L = env
    src = D.ragged_inputs()
    bs, ps = len(D.RAGGED_T), 64
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    vpool, ids = oracle.v_rowmajor_to_pool(src["v_codes"], ps)
    kpool, _ = oracle.k_rowmajor_to_pool(src["k_codes"], ps)
    ids_t = cu(ids.astype(np.int32))
    kp, vp = ops.prepare_cents(cu(src["k_cents"]), cache=False), ops.prepare_cents(cu(src["v_cents"]), cache=False)
    lengths = cu(np.array([[D.RAGGED_T[b], D.RAGGED_R[b], D.RAGGED_START[b], 0] for b in range(bs)], np.int32))
    c0 = D.ragged_case(0, policy)
    assert P.kernel_kind(c0, lib, L) == 1
    try:
        ops.set_force_generic(policy)
        out = ops.pq_decode_attn(cu(src["q"]), cu(kpool), cu(vpool), kp, vp, cu(src["k_res"]), cu(src["v_res"]), 0, M=64, C=256,
                                 n_tokens=D.RAGGED_TMAX, k_page_ids=ids_t, v_page_ids=ids_t, page_size=ps, dev_lengths=lengths)
        torch.cuda.synchronize()
    finally:
        ops.set_force_generic(0)
    assert ops.tail_faults() == 0
    o = out.cpu().numpy()
    for b in range(bs):
        c, one = D.ragged_request(src, b, policy)
        D.check_heads(o[b:b + 1], D.gold(oracle, c, D.request(one, b)), f"ragged {'stream' if policy else 'lean'} request {b} T{c.T} r{c.r}@{c.rs}", "gauss4")


# ---------------------------------------------------------------- f. merge paths ------------------------------------------
@pytest.mark.parametrize("cname", ["lean-d128-M64-ps64-C128", "stream-M32-C256"])
@pytest.mark.parametrize("name", ["descending", "peak:code_last"])
def test_decode_merge_take_over_gives_the_same_bits(name, cname, env, oracle):
    """Policies 4 and 8: the merge helpers give up (every give-up bit preset / through the real atomic path) and the last
    arriver merges every head.  Same partials, same arithmetic: the same bits as policy 0 on the same input, on the lean kernel
    and on the streaming kernel (8 query heads per kv head keep M = 32 there under any policy)."""
    c0 = dataclasses.replace(P.BY_NAME[cname], policy=0)
    assert D.mfma_splits(c0.T_host, c0.bs * c0.nhk, c0.cap) > 1
    base, built = _case(env, oracle, c0, name)
    for policy in (4, 8):
        out = _run(env, dataclasses.replace(c0, policy=policy), built)
        assert np.array_equal(out.view(np.uint16), base.view(np.uint16)), f"{cname} {name}: policy {policy} differs from policy 0"
