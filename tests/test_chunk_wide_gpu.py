"""ops.pq_chunk_attn_wide (csrc/chunk_attn_wide.hip, million_pq_chunk_attn_wide) and DynamicPQCache.extend at nbits 9 .. 12 on the
GPU, against the fp64 model of tests/chunk_wide_model.py.

Bars (the project's, tests/test_chunk_attn_gpu.py and tests/test_attn_wide_gpu.py): rel-L2 < 1e-3 and mean-abs < 1e-3 of fp64 for
every (request, head) on its own, outputs finite.  lse: the uint8 chunk kernel's worst |lse - model| over the matrix's own
inputs with their codes taken below 256 is measured once (u8_lse_worst); the wide call may be off by twice that.  Codes are
uniform in [0, C) and every case asserts that codes >= 256 are among the live ones on both sides."""
import numpy as np
import pytest

from tests import chunk_wide_model as CM

pytestmark = pytest.mark.gpu
REL_TOL = MEAN_ABS_TOL = 1e-3
WIN = {"0": (0, 0), "17": (17, 3), "wrap": (40, 59), "full": (64, 0)}      # (r, resid_start) in a ring of CAP rows: "wrap" runs over its end
CAP = 64


@pytest.fixture(scope="module")
def env():
    import torch
    from million_amd import build, ops
    build.build()
    assert torch.cuda.is_available()
    return torch, ops


def splits(bs, nhk, n_q, G, T):
    """The split count documented in include/million_hip.h (million_chunk_attn_workspace_bytes)."""
    blocks = bs * nhk * -(-n_q * G // 256)
    return max(1, min(-(-256 // blocks), -(-T // 64), 64))


class Case:
    """Live data of one call - codes up to each T_b, the ring span of each window, the first n_q_b query / chunk rows - and two
    ways of filling everything around it: zeros, or what must never reach a product.  rows: one (T, window, n_q) per request."""

    def __init__(self, d, M, C, G, rows, chunk, *, nhk=2, seed=0, code_hi=None):
        rs = np.random.RandomState(seed + d + M + C)
        f = lambda *s: rs.standard_normal(s).astype(np.float16)
        self.d, self.M, self.C, self.G, self.nhk, self.chunk = d, M, C, G, nhk, chunk
        self.bs, self.nh = len(rows), G * nhk
        self.Ts, self.nqs = [r[0] for r in rows], [r[2] for r in rows]
        self.rs, self.ss = [WIN[r[1]][0] for r in rows], [WIN[r[1]][1] for r in rows]
        self.Tb, self.n_q = max(self.Ts), max(self.nqs)
        self.q = f(self.bs, self.nh, self.n_q, d)
        self.k_ch, self.v_ch = (f(self.bs, nhk, self.n_q, d), f(self.bs, nhk, self.n_q, d)) if chunk else (None, None)
        self.k_cents, self.v_cents = f(M, C, d // M), f(M, C, d // M)
        self.k_res, self.v_res = f(self.bs, nhk, CAP, d), f(self.bs, nhk, CAP, d)
        hi = C if code_hi is None else code_hi
        self.k_codes = rs.randint(0, hi, (self.bs, nhk, self.Tb, M)).astype(np.uint16)
        self.v_codes = rs.randint(0, hi, (self.bs, nhk, self.Tb, M)).astype(np.uint16)

    def live_codes_are_wide(self):
        return all(t == 0 or (self.k_codes[b, :, :t].max() >= 256 and self.v_codes[b, :, :t].max() >= 256) for b, t in enumerate(self.Ts))

    def narrow(self):
        """The uint8 twin: the same inputs with the codes taken below 256 and the first 256 entries of every subspace."""
        tw = object.__new__(Case)
        tw.__dict__.update(self.__dict__)
        tw.C, tw.k_codes, tw.v_codes = 256, self.k_codes & 0xFF, self.v_codes & 0xFF
        tw.k_cents, tw.v_cents = np.ascontiguousarray(self.k_cents[:, :256]), np.ascontiguousarray(self.v_cents[:, :256])
        return tw

    def model(self, b=None):
        sl = slice(None) if b is None else slice(b, b + 1)
        pick = lambda x: x[sl]
        return CM.chunk_attn(self.q[sl], self.k_codes[sl], self.v_codes[sl], self.k_cents, self.v_cents, self.k_res[sl], self.v_res[sl],
                             pick(self.rs), T=pick(self.Ts), start=pick(self.ss), k_chunk=None if self.k_ch is None else self.k_ch[sl],
                             v_chunk=None if self.v_ch is None else self.v_ch[sl], n_q=pick(self.nqs))

    # ---- device tensors ----
    def _cents(self, torch, cents, big, poison):
        """big: a view at the front of an allocation of 65536 entries per subspace count whose tail is NaN (zeros when clean):
        an index that was not masked reads NaN inside the allocation, never outside it (test_attn_wide_gpu.Store.cents_dev)."""
        if not big:
            return torch.from_numpy(cents).cuda()
        buf = torch.full((self.M * 65536 * cents.shape[2],), float("nan") if poison else 0.0, dtype=torch.float16, device="cuda")
        view = buf[:cents.size].view(*cents.shape)
        view.copy_(torch.from_numpy(cents))
        return view

    def tensors(self, torch, ops, *, k="rowmajor", v="rowmajor", ps=64, i64=False, poison=False, u8=False, big_cents=False, only=None):
        """u8: uint8 codes and prepared codebooks (the arguments of ops.pq_chunk_attn).  only=b: request b as a batch of one."""
        sl = slice(None) if only is None else slice(only, only + 1)
        bs = len(self.Ts[sl])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        nan = np.float16("nan") if poison else np.float16(0)
        dt = np.uint8 if u8 else np.uint16
        bad = dt(0xFF if u8 else 0xFFFF) if poison else dt(0)
        q, k_res, v_res = self.q[sl].copy(), self.k_res[sl].copy(), self.v_res[sl].copy()
        k_ch, v_ch = (self.k_ch[sl].copy(), self.v_ch[sl].copy()) if self.chunk else (None, None)
        for b, (r, s, nq) in enumerate(zip(self.rs[sl], self.ss[sl], self.nqs[sl])):
            dead = np.setdiff1d(np.arange(CAP), (s + np.arange(r)) % CAP)
            k_res[b, :, dead] = v_res[b, :, dead] = nan
            q[b, :, nq:] = nan
            if self.chunk:
                k_ch[b, :, nq:] = v_ch[b, :, nq:] = nan
        t = dict(q=dev(q), k_ch=None if k_ch is None else dev(k_ch), v_ch=None if v_ch is None else dev(v_ch), k_res=dev(k_res),
                 v_res=dev(v_res), kw={})
        if u8:
            t["k_tab"] = ops.prepare_cents(dev(self.k_cents), cache=False)
            t["v_tab"] = ops.prepare_cents(dev(self.v_cents), cache=False)
        else:
            t["k_tab"], t["v_tab"] = self._cents(torch, self.k_cents, big_cents, poison), self._cents(torch, self.v_cents, big_cents, poison)
        Tb, M, nhk = self.Tb, self.M, self.nhk
        npl = -(-Tb // ps)                                   # pages up to the bound; one more table entry behind them
        n_pool, spare = bs * nhk * npl, 3
        rs = np.random.RandomState(5)
        phys = rs.permutation(n_pool + spare)                # physical page order must not matter
        ids = phys[:n_pool].reshape(bs, nhk, npl)
        ids = np.concatenate([ids, np.zeros((bs, nhk, 1), ids.dtype)], axis=2)
        for b, T in enumerate(self.Ts[sl]):                  # entries past a request's live pages name the spare pages
            live = -(-T // ps)
            ids[b, :, live:] = phys[n_pool + np.arange(npl + 1 - live) % spare]
        for side, codes, lay in (("k", self.k_codes[sl], k), ("v", self.v_codes[sl], v)):
            if lay == "rowmajor":
                arr = np.full((bs, nhk, Tb + 64, M), bad, dt)
                for b, T in enumerate(self.Ts[sl]):
                    arr[b, :, :T] = codes[b, :, :T]
                t[side + "_codes"] = dev(arr)
                continue
            pool = np.full((n_pool + spare, ps, M), bad, dt)
            for b, T in enumerate(self.Ts[sl]):
                for h in range(nhk):
                    for pg in range(-(-T // ps)):
                        n = min(ps, T - pg * ps)
                        pool[ids[b, h, pg], :n] = codes[b, h, pg * ps:pg * ps + n]
            t[side + "_codes"] = dev(pool if side == "k" else pool.transpose(0, 2, 1))
            t["kw"][side + "_page_ids"] = dev(ids.astype(np.int64 if i64 else np.int32))
            t["kw"]["page_size"] = ps
        if "k_page_ids" in t["kw"] and "v_page_ids" in t["kw"]:
            t["kw"]["v_page_ids"] = t["kw"]["k_page_ids"]
        t["lengths"] = dev(np.array([[T, r, s, 0x7EADBEEF] for T, r, s in zip(self.Ts[sl], self.rs[sl], self.ss[sl])], np.int32))
        t["n_q"] = dev(np.array(self.nqs[sl], np.int32))
        t["host"] = (self.Ts[sl][0], self.rs[sl][0], self.ss[sl][0])
        t["bs"] = bs
        return t

    def run(self, torch, ops, t, *, ragged=False, u8=False, poison=False, lse=True, own=True):
        """-> (out, lse) device tensors (lse None when not asked for).  own: out / workspace / lse are this call's, pre-filled with
        NaN when `poison`; the workspace is sized by the documented formula."""
        bs, n_q = t["bs"], self.n_q
        T, r, s = (self.Tb, 0, 0) if ragged else t["host"]
        kw = dict(t["kw"])
        if ragged:
            kw.update(dev_lengths=t["lengths"], dev_n_q=t["n_q"])
        if own:
            S = splits(bs, self.nhk, n_q, self.G, T)
            need = bs * self.nhk * S * n_q * self.G * (self.d + 2) * 4 if S > 1 else 0
            kw["workspace"] = torch.full((max(need, 16),), 0xFF if poison else 0, dtype=torch.uint8, device="cuda")
            kw["out"] = torch.full((bs, n_q, self.nh, self.d), float("nan") if poison else 0.0, dtype=torch.float16, device="cuda").transpose(1, 2)
            if lse:
                kw["lse"] = torch.full((bs, self.nh, n_q), float("nan") if poison else 0.0, dtype=torch.float32, device="cuda")
        elif lse:
            kw["return_lse"] = True
        fn = ops.pq_chunk_attn if u8 else ops.pq_chunk_attn_wide
        got = fn(t["q"], t["k_ch"], t["v_ch"], t["k_codes"], t["v_codes"], t["k_tab"], t["v_tab"], t["k_res"], t["v_res"], r, M=self.M,
                 C=self.C, n_tokens=T, resid_start=s, **kw)
        torch.cuda.synchronize()
        return got if lse else (got, None)


def within_bar(out, ref, what):
    rel, mabs = CM.head_errors(out.float().cpu().numpy(), ref)
    print(f"{what}: worst (request, head) rel-L2 {rel.max():.3e}, mean-abs {mabs.max():.3e}")
    assert np.isfinite(out.float().cpu().numpy()).all(), f"{what}: non-finite output"
    assert np.isfinite(rel).all() and rel.max() < REL_TOL and mabs.max() < MEAN_ABS_TOL, \
        f"{what}: worst rel-L2 {rel.max():.3e} mean-abs {mabs.max():.3e} at {np.unravel_index(rel.argmax(), rel.shape)}"


def same_bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                       b.contiguous().view(torch.int16 if b.dtype == torch.float16 else torch.int32))


# ---------------------------------------------------------------- 1. the matrix ---------------------------------------------
# (d, M, C, G, n_q, T, window, chunk, K layout, V layout, page size, int64 ids): every row sits on an edge - a tile or page edge of T,
# S > 1 (T = 4097), T = 0, one / two query blocks (257 rows and G = 8), an empty / plain / wrapped window, with and without the chunk
MATRIX = [
    (128, 64, 1024, 4, 3, 1000, "17", True, "rowmajor", "rowmajor", 64, False),
    (128, 64, 512, 8, 1, 4097, "wrap", False, "paged", "paged", 64, True),
    (128, 32, 4096, 1, 65, 63, "0", True, "paged", "paged", 32, False),
    (128, 32, 2048, 4, 3, 64, "wrap", True, "rowmajor", "rowmajor", 64, False),
    (128, 64, 1024, 8, 257, 1, "17", True, "paged", "paged", 128, True),
    (128, 32, 512, 1, 3, 4097, "0", False, "paged", "rowmajor", 32, False),
    (128, 64, 2048, 4, 65, 65, "17", True, "paged", "rowmajor", 64, False),
    (64, 32, 1024, 4, 65, 1000, "wrap", True, "rowmajor", "rowmajor", 64, False),
    (64, 16, 4096, 8, 3, 1000, "17", True, "paged", "paged", 64, False),
    (64, 32, 2048, 4, 257, 64, "wrap", False, "rowmajor", "rowmajor", 64, False),
    (64, 16, 512, 1, 1, 0, "17", True, "rowmajor", "rowmajor", 64, False),
    (64, 16, 1024, 8, 3, 4097, "0", True, "paged", "paged", 128, True),
    (128, 32, 4096, 1, 1, 0, "0", True, "paged", "paged", 32, False),
]
ROW_IDS = [f"d{r[0]}-M{r[1]}-C{r[2]}-G{r[3]}-nq{r[4]}-T{r[5]}-w{r[6]}-{'chunk' if r[7] else 'past'}-{r[8][0]}{r[9][0]}{r[10]}" for r in MATRIX]
_cases = {}


def matrix_case(i):
    """Inputs and model of matrix row i, drawn and computed once."""
    if i not in _cases:
        d, M, C, G, n_q, T, win, chunk = MATRIX[i][:8]
        c = Case(d, M, C, G, [(T, win, n_q)] * (2 if n_q <= 3 else 1), chunk, seed=i)
        _cases[i] = (c, c.model())
    return _cases[i]


@pytest.fixture(scope="module")
def u8_lse_worst(env):
    """The uint8 chunk kernel's worst |lse - model| over the matrix's inputs with codes < 256 (Case.narrow)."""
    torch, ops = env
    worst = 0.0
    for i, row in enumerate(MATRIX):
        tw = matrix_case(i)[0].narrow()
        _, lse = tw.run(torch, ops, tw.tensors(torch, ops, k=row[8], v=row[9], ps=row[10], i64=row[11], u8=True), u8=True)
        worst = max(worst, CM.lse_error(lse.cpu().numpy(), tw.model()[1]))
    print(f"uint8 chunk kernel, worst |lse - model| over the matrix: {worst:.3e}")
    assert worst > 0
    return worst


@pytest.mark.parametrize("i", range(len(MATRIX)), ids=ROW_IDS)
def test_matrix(env, u8_lse_worst, i):
    torch, ops = env
    c, (ref, ref_l) = matrix_case(i)
    assert c.live_codes_are_wide()
    k, v, ps, i64 = MATRIX[i][8:]
    out, lse = c.run(torch, ops, c.tensors(torch, ops, k=k, v=v, ps=ps, i64=i64), own=False)
    within_bar(out, ref, ROW_IDS[i])
    err = CM.lse_error(lse.cpu().numpy(), ref_l)
    print(f"{ROW_IDS[i]}: worst |lse - model| {err:.3e} (uint8 kernel over the matrix: {u8_lse_worst:.3e})")
    assert err <= 2 * u8_lse_worst


# ---------------------------------------------------------------- 2. the bitwise twin of the uint8 kernel -------------------
RAGGED_ROWS = [(4097, "17", 5), (1000, "wrap", 0), (64, "0", 3), (0, "17", 1)]
TWINS = {"S1": [(64, "17", 5)] * 2, "split": [(4097, "wrap", 5)], "ragged": RAGGED_ROWS}


@pytest.mark.parametrize("d,M", [(128, 64), (64, 16)], ids=["d128-dm2", "d64-dm4"])
@pytest.mark.parametrize("form", list(TWINS))
def test_bitwise_twin_of_the_uint8_kernel(env, form, d, M):
    """Codes < 256 widened to uint16 and a C = 512 table whose entries [:, :256] are a C = 256 table (the rest random): the wide
    call is the uint8 call, bit for bit - tile order, masks, split cut and merge are the trusted kernel's."""
    torch, ops = env
    rows = TWINS[form]
    c = Case(d, M, 512, 4, rows, True, seed=7, code_hi=256)
    tw = c.narrow()
    assert (splits(len(rows), 2, 5, 4, c.Tb) > 1) == (form != "S1")
    lay = dict(k="paged", v="paged", ps=64) if d == 128 else dict(k="rowmajor", v="paged", ps=32)
    ragged = form == "ragged"
    out_w, lse_w = c.run(torch, ops, c.tensors(torch, ops, **lay), ragged=ragged)
    out_8, lse_8 = tw.run(torch, ops, tw.tensors(torch, ops, u8=True, **lay), ragged=ragged, u8=True)
    assert same_bits(out_w, out_8) and same_bits(lse_w, lse_8)
    assert out_w.any() and torch.isfinite(out_w).all()


# ---------------------------------------------------------------- 3. poison --------------------------------------------------
@pytest.mark.parametrize("lay", [dict(k="rowmajor", v="rowmajor"), dict(k="paged", v="paged", ps=32)], ids=["rowmajor", "paged32"])
@pytest.mark.parametrize("form", ["lockstep", "ragged"])
def test_poison_moves_no_bit(env, form, lay):
    """The same live data inside zeros and inside poison: 0xFFFF code words past T (row-major padding, page tails), 0xFFFF unused
    pool pages, table entries past each request's live pages that name such pages, NaN window rows outside the ring span, NaN q
    and chunk rows at or past dev_n_q[b], a NaN workspace, out and lse, and codebooks at the front of 65536-entry allocations
    with NaN tails (an index without its & (C - 1) reads NaN)."""
    torch, ops = env
    rows = RAGGED_ROWS if form == "ragged" else [(1000, "wrap", 5)] * 2
    c = Case(128, 64, 1024, 4, rows, True, seed=11)
    assert c.live_codes_are_wide()
    ragged = form == "ragged"
    clean = c.run(torch, ops, c.tensors(torch, ops, big_cents=True, **lay), ragged=ragged)
    dirty = c.run(torch, ops, c.tensors(torch, ops, big_cents=True, poison=True, **lay), ragged=ragged, poison=True)
    assert torch.isfinite(dirty[0]).all() and not torch.isnan(dirty[1]).any(), "poison reached the output"
    assert same_bits(clean[0], dirty[0]) and same_bits(clean[1], dirty[1])
    ref, ref_l = c.model()
    within_bar(clean[0], ref, f"{form} clean")
    CM.lse_error(clean[1].cpu().numpy(), ref_l)      # the -inf rows are the model's


# ---------------------------------------------------------------- 4. ragged equals alone -------------------------------------
# A request alone (batch 1, host lengths) is cut into S' = min(ceil(256 / nh_k), ceil(T_b / 64), 64) splits, the ragged launch
# into S = min(ceil(256 / (bs nh_k)), ceil(bound / 64), 64): the bits can only agree where S' = S.  "S1": a bound of one tile
# gives S = S' = 1 whatever T_b is; "split": bound 1000 is 16 tiles, and so are 990 and 961 tokens: S = S' = 16.
ALONE = {"S1": [(64, "17", 5), (33, "wrap", 3), (1, "0", 5), (0, "17", 1), (40, "17", 0)],
         "split": [(1000, "17", 5), (990, "wrap", 3), (961, "0", 5), (1000, "wrap", 0)]}


@pytest.mark.parametrize("form", list(ALONE))
def test_ragged_equals_alone(env, form):
    torch, ops = env
    rows = ALONE[form]
    c = Case(128, 32, 2048, 4, rows, True, seed=13)
    for b, (T, _, _) in enumerate(rows):
        assert splits(1, 2, 5, 4, T) == splits(len(rows), 2, 5, 4, c.Tb) or rows[b][2] == 0
    lay = dict(k="paged", v="paged", ps=32)
    out, lse = c.run(torch, ops, c.tensors(torch, ops, poison=True, **lay), ragged=True, poison=True)
    for b, (T, win, nq) in enumerate(rows):
        assert not out[b, :, nq:].any() and torch.isneginf(lse[b, :, nq:]).all(), b      # rows >= dev_n_q[b]: zeros, lse -inf
        if nq == 0:
            continue
        one = Case.__new__(Case)
        one.__dict__.update(c.__dict__)
        one.n_q = nq                                                                    # its own rows only
        one.q, one.k_ch, one.v_ch = c.q[:, :, :nq], c.k_ch[:, :, :nq], c.v_ch[:, :, :nq]
        o1, l1 = one.run(torch, ops, one.tensors(torch, ops, only=b, **lay))
        assert same_bits(out[b:b + 1, :, :nq], o1) and same_bits(lse[b:b + 1, :, :nq], l1), b


def test_graph_replay_follows_the_lengths(env):
    """One captured ragged call (the attention kernel and the merge on one stream) replayed after dev_lengths / dev_n_q changed."""
    torch, ops = env
    full = [(1000, "full", 5)] * 2
    c = Case(128, 64, 1024, 4, full, False, seed=17)
    t = c.tensors(torch, ops, k="paged", v="paged", ps=64)      # every code up to the bound and every window row is live in some state
    states = [[(63, 5, 0, 5), (1000, 0, 0, 3)], [(65, 64, 40, 2), (1000, 17, 3, 5)], [(128, 0, 0, 0), (936, 64, 63, 5)]]
    S = splits(2, 2, 5, 4, 1000)
    ws = torch.empty(2 * 2 * S * 5 * 4 * (128 + 2) * 4, dtype=torch.uint8, device="cuda")
    out = torch.zeros(2, 5, c.nh, 128, dtype=torch.float16, device="cuda").transpose(1, 2)
    lse = torch.zeros(2, c.nh, 5, dtype=torch.float32, device="cuda")
    lengths, n_q = t["lengths"].clone(), t["n_q"].clone()
    call = lambda: ops.pq_chunk_attn_wide(t["q"], None, None, t["k_codes"], t["v_codes"], t["k_tab"], t["v_tab"], t["k_res"], t["v_res"], 0,
                                          M=c.M, C=c.C, n_tokens=1000, dev_lengths=lengths, dev_n_q=n_q, workspace=ws, out=out, lse=lse,
                                          **t["kw"])
    call()      # eager once: module load
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for rows in states:
        lengths.copy_(torch.tensor([[T, r, s, 0] for T, r, s, _ in rows], dtype=torch.int32))
        n_q.copy_(torch.tensor([r[3] for r in rows], dtype=torch.int32))
        out.fill_(float("nan"))
        lse.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        ref, ref_l = CM.chunk_attn(c.q, c.k_codes, c.v_codes, c.k_cents, c.v_cents, c.k_res, c.v_res, [r[1] for r in rows],
                                   T=[r[0] for r in rows], start=[r[2] for r in rows], n_q=[r[3] for r in rows])
        within_bar(out, ref, f"replay {rows}")
        CM.lse_error(lse.cpu().numpy(), ref_l)
        for b, r in enumerate(rows):
            assert not out[b, :, r[3]:].any()


# ---------------------------------------------------------------- 5. out with lse is out without; the lse ---------------------
@pytest.mark.parametrize("i", [0, 1, 8, 11], ids=[ROW_IDS[i] for i in (0, 1, 8, 11)])
def test_out_with_lse_is_out_without(env, i):
    torch, ops = env
    c, _ = matrix_case(i)
    k, v, ps, i64 = MATRIX[i][8:]
    t = c.tensors(torch, ops, k=k, v=v, ps=ps, i64=i64)
    with_lse, _ = c.run(torch, ops, t)
    without, none = c.run(torch, ops, t, lse=False)
    assert none is None and same_bits(with_lse, without)


def test_a_row_that_sees_no_key(env):
    torch, ops = env
    c = Case(128, 64, 1024, 4, [(0, "0", 3)] * 2, False, seed=19)
    for lay in (dict(), dict(k="paged", v="paged", ps=64)):
        out, lse = c.run(torch, ops, c.tensors(torch, ops, poison=True, **lay), poison=True)
        assert not out.any() and torch.isneginf(lse).all()


# ---------------------------------------------------------------- 6. a live wide PagedPQCache, read only ---------------------
def test_against_a_live_paged_cache(env, oracle):
    """Two slots at different lengths, decoded with device lengths across a flush (slot 0's window wraps), then read by the chunk
    call through the cache's own pools, page table, length rows and windows.  The model is built from host copies of that state;
    the cache is not touched.  The flush of a cache with uint16 codes serves requests in lockstep only, so the
    slots cross it together and slot 1 gets its own length behind it: release, prefill_request of a shorter prompt, more steps."""
    torch, ops = env
    from million_amd.pq_cache import PagedPQCache
    bs, nh, nhk, d, M, nbits, ps, win = 2, 8, 2, 128, 64, 10, 32, 64
    rs = np.random.RandomState(23)
    f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float16)).cuda()
    cache = PagedPQCache(bs=bs, nh=nh, num_key_value_heads=nhk, M=M, layer_num=1, nbits=nbits, dtype=torch.uint16, d=d, page_size=ps,
                         extended_residual_size=win, max_tokens=512)
    k_cents, v_cents = f(M, 2 ** nbits, d // M), f(M, 2 ** nbits, d // M)
    cache.set_cent(k_cents, v_cents)
    def steps(n):
        for _ in range(n):
            cache.begin_step(use_dev_lengths=True)
            cache.decoding_with_pages(f(bs, nh, 1, d), f(bs, nhk, 1, d), f(bs, nhk, 1, d), 0, use_dev_lengths=True)

    for b in range(bs):
        cache.prefill_request(b, f(1, nh, 70, d), f(1, nhk, 70, d), f(1, nhk, 70, d), 0)
    steps(win + 3)
    cache.release(1)
    cache.prefill_request(1, f(1, nh, 45, d), f(1, nhk, 45, d), f(1, nhk, 45, d), 0)
    steps(3)
    torch.cuda.synchronize()
    rows = cache.lengths[0].cpu().numpy()
    assert rows[:, :3].tolist() == [[70 + ps, win - ps + 6, ps], [45, 3, 0]] and rows[0, 1] + rows[0, 2] > win      # flushed; slot 0's ring wraps
    snap = lambda: [a.copy() for a in cache.host_state()] + [cache.lengths[0].clone(), cache.page_ids[0].clone(), cache.key_page_pool.clone(),
                                                            cache.value_page_pool.clone(), cache.key_residual_cache[0].clone(),
                                                            cache.value_residual_cache[0].clone()]
    same = lambda x, y: all(torch.equal(a, b) if isinstance(a, torch.Tensor) else np.array_equal(a, b) for a, b in zip(x, y))
    before = snap()
    # host copies of the state: the codes of each request through its table
    ids = cache.page_ids[0].cpu().numpy()
    kp = cache.key_page_pool.view(torch.int16).cpu().numpy().view(np.uint16)
    vp = cache.value_page_pool.view(torch.int16).cpu().numpy().view(np.uint16)
    Tb = int(rows[:, 0].max())
    kc, vc = np.zeros((bs, nhk, Tb, M), np.uint16), np.zeros((bs, nhk, Tb, M), np.uint16)
    for b in range(bs):
        for h in range(nhk):
            for t in range(int(rows[b, 0])):
                kc[b, h, t], vc[b, h, t] = kp[ids[b, h, t // ps], t % ps], vp[ids[b, h, t // ps], :, t % ps]
    assert kc.max() >= 256 and vc.max() >= 256
    k_res, v_res = cache.key_residual_cache[0].cpu().numpy(), cache.value_residual_cache[0].cpu().numpy()
    bound = cache.page_ids[0].shape[2] * ps
    q, k_ch, v_ch = f(bs, nh, 4, d), f(bs, nhk, 4, d), f(bs, nhk, 4, d)
    for chunk in (False, True):
        out, lse = ops.pq_chunk_attn_wide(q, k_ch if chunk else None, v_ch if chunk else None, cache.key_page_pool, cache.value_page_pool,
                                          cache.key_cent, cache.value_cent, cache.key_residual_cache[0], cache.value_residual_cache[0], 0,
                                          M=M, C=2 ** nbits, n_tokens=bound, k_page_ids=cache.page_ids[0], v_page_ids=cache.page_ids[0],
                                          page_size=ps, dev_lengths=cache.lengths[0], return_lse=True)
        torch.cuda.synchronize()
        ref, ref_l = CM.chunk_attn(q.cpu().numpy(), kc, vc, k_cents.cpu().numpy(), v_cents.cpu().numpy(), k_res, v_res, rows[:, 1],
                                   T=rows[:, 0], start=rows[:, 2], k_chunk=k_ch.cpu().numpy() if chunk else None,
                                   v_chunk=v_ch.cpu().numpy() if chunk else None)
        within_bar(out, ref, f"live cache, chunk={chunk}")
        CM.lse_error(lse.cpu().numpy(), ref_l)
    assert same(before, snap())


# ---------------------------------------------------------------- 7. DynamicPQCache.extend at nbits 9 .. 12 -------------------
@pytest.mark.parametrize("nbits,M", [(10, 64), (12, 32)])
def test_dynamic_cache_extend(env, oracle, nbits, M):
    """prefill 50 -> extend 5 -> extend 70 -> extend 1: every output within the bar of the model over oracle.pq_encode's codes of all
    earlier rows, the store bit-exact oracle.pq_encode of the concatenated rows, the last output within the bar of dense attention
    over update()'s dequantised K/V on a twin cache."""
    torch, ops = env
    from million_amd.pq_cache import DynamicPQCache
    bs, nhk, G, d, C = 2, 2, 4, 128, 2 ** nbits
    nh = nhk * G
    rs = np.random.RandomState(nbits)
    h = lambda *s: rs.standard_normal(s).astype(np.float16)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ck, cv = h(M, C, d // M), h(M, C, d // M)
    steps = [50, 5, 70, 1]
    n_all = sum(steps)
    K, V, Q = h(bs, nhk, n_all, d), h(bs, nhk, n_all, d), h(bs, nh, n_all, d)
    Kc, Vc = oracle.pq_encode(K, ck), oracle.pq_encode(V, cv)
    assert Kc.dtype == np.uint16 and Kc.max() >= 256 and Vc.max() >= 256
    mk = lambda: DynamicPQCache(bs=bs, nh=nh, num_key_value_heads=nhk, M=M, layer_num=1, d=d, nbits=nbits, max_tokens=256)
    cache, twin = mk(), mk()
    for c in (cache, twin):
        c.set_cent(g(ck), g(cv))
    empty = np.zeros((bs, nhk, 1, d), np.float16)
    t0 = 0
    for i, n in enumerate(steps):
        sl = slice(t0, t0 + n)
        q, k, v = g(Q[:, :, sl]), g(K[:, :, sl]), g(V[:, :, sl])
        out = cache.prefill(q, k, v, 0) if i == 0 else cache.extend(q, k, v, 0)
        torch.cuda.synchronize()
        assert cache._T[0] == t0 + n and cache.residualed_tokens[0] == 0
        if i:
            ref, _ = CM.chunk_attn(Q[:, :, sl], Kc[:, :, :t0], Vc[:, :, :t0], ck, cv, empty, empty, 0, k_chunk=K[:, :, sl], v_chunk=V[:, :, sl])
            within_bar(out, ref, f"nbits {nbits}: extend {n} behind {t0}")
        if i < len(steps) - 1:
            twin.update(k, v, 0)
        else:      # the dense route these codes had: the whole past as fp16
            Kd, Vd = twin.update(k, v, 0)
            assert Kd.shape[2] == n_all
            Kd, Vd = Kd.double().cpu().numpy(), Vd.double().cpu().numpy()
            s = np.einsum("bhd,bhnd->bhn", Q[:, :, -1].astype(np.float64), np.repeat(Kd, G, axis=1)) / np.sqrt(d)
            p = np.exp(s - s.max(axis=-1, keepdims=True))
            dense = np.einsum("bhn,bhnd->bhd", p / p.sum(axis=-1, keepdims=True), np.repeat(Vd, G, axis=1))[:, :, None]
            within_bar(out, dense, f"nbits {nbits}: extend 1 against update()")
        t0 += n
    np.testing.assert_array_equal(cache.key_cache[0].view(torch.int16).cpu().numpy().view(np.uint16), Kc)
    np.testing.assert_array_equal(cache.value_cache[0].view(torch.int16).cpu().numpy().view(np.uint16), Vc)
