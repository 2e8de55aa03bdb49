"""GPU tests of the flash family - prefill_attn_kernel<128|64>, prefill_attn_pipe_kernel (csrc/prefill.hip), chunk_attn_kernel and
chunk_merge_kernel (csrc/chunk_attn.hip), all on csrc/flash_tile.h - against fp64, with the project's bar of rel-L2 < 1e-3
applied to EVERY output row (tests/flash_inputs.py: check_rows) on inputs shaped like attention in a language model: logit
spreads of 1 .. 8, outlier channels, a sink with a recency ramp, staircases of rising scores, rows whose tail is fp16-subnormal,
scaled V; every grouping of query heads; lengths at every tile and query-block edge; live data surrounded by NaN.
tests/test_flash_numerics_host.py shows on the CPU that these inputs leave a correct kernel half the bar of room."""
import ctypes

import numpy as np
import pytest

from tests import flash_inputs as F
from tests import test_chunk_attn_gpu as C

pytestmark = pytest.mark.gpu

SHAPES = [(1024, 1024, 0, True), (333, 1500, 1167, True), (200, 777, 0, False)]      # (n_q, n_kv, q_pos0, causal)
SHAPE_IDS = ["1024sq", "333at1167", "200x777-noncausal"]
GROUPS = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16]
SENTINEL = -1234.0
PAD = 64      # rows of NaN / sentinel before and after the live rows: a whole key tile, so that a kernel that forgot a clamp reads NaN, not foreign memory


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    return torch, ops


def _cu(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _prefill(env, q, k, v, q_pos0, causal, policy):
    """policy 0: the default kernels (pipelined at d = 128); 64: the plain tile loop at d = 128 too."""
    torch, ops = env
    try:
        ops.set_force_generic(policy)
        out = ops.prefill_attn(_cu(torch, q), _cu(torch, k), _cu(torch, v), causal=causal, q_pos0=q_pos0)
        torch.cuda.synchronize()
    finally:
        ops.set_force_generic(0)
    return out.cpu().numpy()


def _prefill_all_forms(env, name, bs, nh, nh_k, n_q, n_kv, q_pos0, causal, what):
    """The three prompt-attention kernels on family `name`: pipelined and plain at d = 128 (one fp64 reference), d = 64."""
    for d, policies in ((128, (0, 64)), (64, (0,))):
        q, k, v = F.prefill_inputs(name, bs, nh, nh_k, n_q, n_kv, d)
        gold = F.prefill_gold(q, k, v, q_pos0, causal)
        for pol in policies:
            form = {(128, 0): "pipelined", (128, 64): "plain", (64, 0): "d64"}[d, pol]
            F.check_rows(_prefill(env, q, k, v, q_pos0, causal, pol), gold, f"prefill {form} {name} {what}", unit=F.v_unit(name))


# ---------------------------------------------------------------- 1. numerics: prompt attention -------------------------
@pytest.mark.parametrize("nh,nh_k", [(32, 8), (8, 8)], ids=["gqa32-8", "gqa8-8"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_prefill_rows_on_llm_shaped_inputs(name, shape, nh, nh_k, env):
    n_q, n_kv, q_pos0, causal = shape
    _prefill_all_forms(env, name, 1, nh, nh_k, n_q, n_kv, q_pos0, causal, f"{n_q}x{n_kv}@{q_pos0} {nh}/{nh_k}")


# ---------------------------------------------------------------- 2. numerics: chunk attention --------------------------
def _splits(st, d, nh, nh_k, n_q):
    """The number of splits the library will use (from its workspace formula)."""
    from million_amd import _lib
    desc = _lib.ChunkAttnDesc()
    desc.struct_size = ctypes.sizeof(_lib.ChunkAttnDesc)
    desc.bs, desc.nh, desc.nh_k, desc.d, desc.n_q, desc.n_tokens = st["q"].shape[0], nh, nh_k, d, n_q, st["k_codes"].shape[2]
    ws = _lib.load().million_chunk_attn_workspace_bytes(ctypes.byref(desc))
    return max(1, ws // (desc.bs * nh_k * n_q * (nh // nh_k) * (d + 2) * 4))


WINDOW = (100, 128, 90)      # r, ring capacity, first row: the window wraps after 38 rows
# (d, M, C, G, n_q, T, chunk, bs, nh_k, layout, page size, splits)
CHUNK_BASE = [
    (128, 64, 256, 4, 96, 64, True, 1, 2, "rowmajor", 0, 1),
    (128, 64, 128, 4, 512, 1000, True, 4, 8, "paged", 64, 1),
    (128, 32, 256, 4, 96, 1000, True, 1, 2, "paged", 32, 16),
    (128, 16, 256, 4, 33, 4097, True, 1, 2, "paged", 128, 64),
    (64, 32, 128, 4, 96, 1000, False, 1, 2, "rowmajor", 0, 16),
]
# one M per d_m form, both codebook sizes, with and without the chunk
CHUNK_FORMS = [(d, M, Cc, 4, 96, 1000, i % 2 == 0, 1, 2, "rowmajor", 0, 16)
               for i, (d, M, Cc) in enumerate((d, M, Cc) for d, M in ((128, 64), (128, 32), (128, 16), (64, 64), (64, 32), (64, 16))
                                              for Cc in ((256, 128) if M != 32 else (128, 256)))]


def _chunk_case(env, oracle, name, case, peak=None):
    torch, ops = env
    d, M, Cc, G, n_q, T, chunk, bs, nh_k, layout, ps, S = case
    r, cap, rstart = WINDOW
    st = F.chunk_inputs(name, bs, G * nh_k, nh_k, d, M, Cc, n_q, T, r, cap, rstart, chunk, peak=peak)
    assert _splits(st, d, G * nh_k, nh_k, n_q) == S
    out = C._run(torch, ops, oracle, st, M, Cc, layout, ps, False)
    what = f"chunk d{d} S{'=1' if S == 1 else '>1'} {'peak_in:' + peak if peak else name} M{M} C{Cc} T{T} n_q{n_q}"
    F.check_rows(out, F.chunk_gold(oracle, st), what, unit=F.v_unit(name))


_ids = lambda cases: ["-".join(map(str, c)) for c in cases]


@pytest.mark.parametrize("case", CHUNK_BASE, ids=_ids(CHUNK_BASE))
@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_chunk_rows_on_llm_shaped_inputs(name, case, env, oracle):
    _chunk_case(env, oracle, name, case)


@pytest.mark.parametrize("case", CHUNK_FORMS, ids=_ids(CHUNK_FORMS))
def test_chunk_rows_every_dequant_form(case, env, oracle):
    _chunk_case(env, oracle, "gauss4", case)


PEAK_CASES = [(p, c) for c in CHUNK_BASE[:4] + CHUNK_FORMS for p in F.PEAKS if c[6] or p != "chunk_row"]


@pytest.mark.parametrize("peak,case", PEAK_CASES, ids=[p + "-" + "-".join(map(str, c)) for p, c in PEAK_CASES])
def test_chunk_rows_with_a_dominating_key(peak, case, env, oracle):
    """One key holds nearly all the mass of every row that sees it: in the first or the last code tile (one split's maximum
    dwarfs the others in the merge), in the window right after the ring wraps, or in the chunk (rows before it do not see it)."""
    _chunk_case(env, oracle, "gauss1", case, peak=peak)


# ---------------------------------------------------------------- 3. structure --------------------------------------------
@pytest.mark.parametrize("G", GROUPS)
def test_prefill_every_head_grouping_in_a_batch(G, env):
    """nh / nh_k = G gives hpw = the largest of 8, 4, 2, 1 dividing G and G / hpw head groups; bs = 3 with q_pos0 > 0."""
    _prefill_all_forms(env, "gauss1", 3, 2 * G, 2, 150, 270, 120, True, f"G{G} bs3")


@pytest.mark.parametrize("n_kv", [100, 149, 150, 151, 230])
@pytest.mark.parametrize("G", [1, 4, 6])
def test_prefill_keys_short_of_and_past_the_last_diagonal(G, n_kv, env):
    """n_q = 100 rows at positions 50 .. 149: with fewer keys than that the limit of late rows is clamped to the last key,
    with more the keys behind the last diagonal must be ignored."""
    _prefill_all_forms(env, "gauss1", 2, 2 * G, 2, 100, n_kv, 50, True, f"G{G} n_kv{n_kv} rows at 50..149")


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "noncausal"])
@pytest.mark.parametrize("n_kv", [63, 64, 65, 127, 128, 129, 191, 193])
def test_prefill_key_counts_at_tile_edges(n_kv, causal, env):
    n_q = 40
    _prefill_all_forms(env, "gauss1", 2, 8, 2, n_q, n_kv, n_kv - n_q if causal else 0, causal, f"n_kv{n_kv} {'causal' if causal else 'all keys'}")


@pytest.mark.parametrize("G,QB", [(8, 32), (4, 64), (2, 128), (1, 256), (3, 256), (12, 64)])
@pytest.mark.parametrize("off", [-1, 0, 1])
def test_prefill_row_counts_at_query_block_edges(G, QB, off, env):
    """A workgroup holds QB = 256 / hpw rows of each of its heads."""
    n_q = QB + off
    _prefill_all_forms(env, "gauss1", 2, 2 * G, 2, n_q, n_q, 0, True, f"G{G} n_q{n_q}")


@pytest.mark.parametrize("d,M", [(128, 64), (64, 32)])
@pytest.mark.parametrize("G", GROUPS)
def test_chunk_every_head_grouping_in_a_batch(G, d, M, env, oracle):
    """rho = i G + g: a wave's 32 flattened rows cover several query indices unless G is a multiple of 32; its causal limit is per
    lane, the tiles it walks come from the integer divisions wave_i_hi and wg_i_hi.  n_q = 70 puts the chunk's second tile in
    reach of only the last rows."""
    torch, ops = env
    r, cap, rstart = WINDOW
    st = F.chunk_inputs("gauss1", 3, 2 * G, 2, d, M, 256, 70, 200, r, cap, rstart, True)
    out = C._run(torch, ops, oracle, st, M, 256, "rowmajor", 0, False)
    F.check_rows(out, F.chunk_gold(oracle, st), f"chunk d{d} structure G{G} bs3")


# ---------------------------------------------------------------- 4. poisoned surroundings --------------------------------
def _embed(torch, a, fill, pad=PAD, gap=24):
    """a (bs, h, n, d) as a strided view into a larger allocation filled with `fill`: `pad` rows before and after every head's
    rows and `gap` elements behind every row.  -> (allocation, view)"""
    bs, h, n, d = a.shape
    buf = torch.full((bs, h, n + 2 * pad, d + gap), fill, dtype=torch.float16, device="cuda")
    view = buf[:, :, pad:pad + n, :d]
    view.copy_(a)
    return buf, view


def _out_buffer(torch, shape, pad=PAD, gap=24):
    bs, h, n, d = shape
    buf = torch.full((bs, h, n + 2 * pad, d + gap), SENTINEL, dtype=torch.float16, device="cuda")
    return buf, buf[:, :, pad:pad + n, :d]


def _sentinels_untouched(torch, buf, shape, pad=PAD):
    bs, h, n, d = shape
    outside = torch.ones(buf.shape, dtype=torch.bool, device="cuda")
    outside[:, :, pad:pad + n, :d] = False
    return bool((buf.view(torch.int16)[outside] == torch.tensor(SENTINEL, dtype=torch.float16).view(torch.int16).item()).all())


@pytest.mark.parametrize("d,policy", [(128, 0), (128, 64), (64, 0)], ids=["pipelined", "plain", "d64"])
@pytest.mark.parametrize("G,n_q,n_kv,q_pos0,causal", [(4, 130, 200, 70, True), (6, 65, 65, 0, True), (1, 257, 300, 10, True),
                                                     (8, 40, 129, 0, False)])
def test_prefill_reads_and_writes_only_its_own_rows(G, n_q, n_kv, q_pos0, causal, d, policy, env):
    """q, k, v are views with a row stride > d into allocations that hold NaN in the gaps and in the rows before the first and
    after the last row; out is a view into an allocation full of a sentinel.  The output is bitwise what zeros in place of the
    NaN give, every row matches fp64, and no sentinel outside out's (bs, nh, n_q, d) elements has moved."""
    torch, ops = env
    q, k, v = F.prefill_inputs("gauss1", 2, 2 * G, 2, n_q, n_kv, d)
    gold = F.prefill_gold(q, k, v, q_pos0, causal)
    got = []
    try:
        ops.set_force_generic(policy)
        for fill in (0.0, float("nan")):
            views = [_embed(torch, torch.from_numpy(a).cuda(), fill)[1] for a in (q, k, v)]
            obuf, out = _out_buffer(torch, q.shape)
            ops.prefill_attn(*views, causal=causal, q_pos0=q_pos0, out=out)
            torch.cuda.synchronize()
            assert _sentinels_untouched(torch, obuf, q.shape), "a sentinel outside out moved"
            got.append(out.contiguous().cpu())
    finally:
        ops.set_force_generic(0)
    assert torch.equal(got[0].view(torch.int16), got[1].view(torch.int16)), "NaN around the live rows changed the output"
    F.check_rows(got[1].numpy(), gold, f"prefill poisoned G{G} n_q{n_q} n_kv{n_kv} d{d} policy {policy}")


class _EmbeddingOps:
    """ops, with pq_chunk_attn's q, chunk K / V and out moved into poisoned / sentinel-filled allocations (C._run builds the
    code and window sides, poisoned by its own poison=True)."""

    def __init__(self, torch, ops, fill):
        self.torch, self.ops, self.fill = torch, ops, fill

    def prepare_cents(self, *a, **kw):
        return self.ops.prepare_cents(*a, **kw)

    def pq_chunk_attn(self, q, k_chunk, v_chunk, *a, **kw):
        emb = lambda t: None if t is None else _embed(self.torch, t, self.fill)[1]
        self.obuf, out = _out_buffer(self.torch, q.shape)
        self.ops.pq_chunk_attn(emb(q), emb(k_chunk), emb(v_chunk), *a, out=out, **kw)
        return out.contiguous()


@pytest.mark.parametrize("d,M,Cc,layout,T,chunk", [(128, 64, 128, "paged", 1000, True), (128, 32, 256, "rowmajor", 40, True),
                                                  (64, 64, 128, "rowmajor", 1000, False), (64, 16, 256, "paged", 4097, True)])
def test_chunk_reads_and_writes_only_its_own_rows(d, M, Cc, layout, T, chunk, env, oracle):
    """The same for chunk attention: 0xFF code bytes past T and in unused pages, NaN window rows outside the ring's valid span,
    NaN around q and the chunk's K / V, a sentinel around out; S = 1 (T = 40) and S > 1."""
    torch, ops = env
    st = F.chunk_inputs("gauss1", 2, 10, 2, d, M, Cc, 70, T, 40, 64, 50, chunk)
    got = []
    for poison in (False, True):
        eo = _EmbeddingOps(torch, ops, float("nan") if poison else 0.0)
        out = C._run(torch, eo, oracle, st, M, Cc, layout, 64, False, poison=poison)
        assert _sentinels_untouched(torch, eo.obuf, st["q"].shape), "a sentinel outside out moved"
        got.append(out)
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), "poison around the live data changed the output"
    F.check_rows(got[1], F.chunk_gold(oracle, st), f"chunk poisoned d{d} M{M} C{Cc} {layout} T{T}")


# ---------------------------------------------------------------- 5. long rows --------------------------------------------
def test_prefill_32k_rows_at_logit_spread_4(env):
    """(1, 32, 8, 32768, 128) with logits of standard deviation 4: 64 rows of every head - the first rows, rows on both sides of key
    tile (64), query block (128 at G = 4) and far edges, random rows - each against fp64."""
    torch, ops = env
    n = 32768
    g = torch.Generator(device="cuda").manual_seed(11)
    q = (2.0 * torch.randn(1, 32, n, 128, generator=g, device="cuda")).half()      # q, k ~ N(0, 2): logits ~ N(0, 4)
    k = (2.0 * torch.randn(1, 8, n, 128, generator=g, device="cuda")).half()
    v = torch.randn(1, 8, n, 128, generator=g, device="cuda").half()
    out = ops.prefill_attn(q, k, v)
    torch.cuda.synchronize()
    edges = [0, 1, 31, 32, 63, 64, 65, 127, 128, 129, 255, 256, 4095, 4096, 16383, 16384, n - 129, n - 128, n - 65, n - 64, n - 2, n - 1]
    more = [int(i) for i in np.random.RandomState(3).choice(n, 64, replace=False) if i not in edges]
    rows = np.sort(np.r_[edges, more[:64 - len(edges)]])
    gold = F.prefill_gold(q[:, :, rows].cpu().numpy(), k.cpu().numpy(), v.cpu().numpy(), rows=rows, sliced=True)
    F.check_rows(out[:, :, rows].cpu().numpy(), gold, "prefill pipelined gauss4 32k sampled rows", rows=rows)
    del q, k, v, out
    torch.cuda.empty_cache()
