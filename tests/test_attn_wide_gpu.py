"""ops.pq_decode_attn_wide (csrc/attn_wide.hip) on the GPU against the fp64 model of tests/wide_model.py.

The bar is the project's: rel-L2 < 1e-3 and mean-abs < 1e-3 of fp64 for every head on its own.  Codes are uniform in [0, C) and every
case asserts that codes >= 256 are among the live ones.  lse: lse_ref.LSE_TOL, as tests/test_attn_lse_gpu.py."""
import numpy as np
import pytest

from tests import lse_ref as R
from tests import wide_model as W

pytestmark = pytest.mark.gpu
REL_TOL = MEAN_ABS_TOL = 1e-3


@pytest.fixture(scope="module")
def env():
    import torch
    from million_amd import build, ops
    build.build()
    assert torch.cuda.is_available()
    return torch, ops


class Store:
    """Random inputs of one shape: row-major codes of T_max tokens scattered into shuffled physical pages, a window, codebooks."""

    def __init__(self, torch, d, M, C, ps, G, *, bs=2, nhk=2, T_max=1029, cap=128, seed=0, spare_pages=3, cents_alloc=None):
        rs = np.random.RandomState(seed + d + M + C)
        self.torch, self.d, self.M, self.C, self.ps, self.G, self.bs, self.nhk, self.cap = torch, d, M, C, ps, G, bs, nhk, cap
        self.nh, dm = nhk * G, d // M
        self.q = rs.standard_normal((bs, self.nh, 1, d)).astype(np.float16)
        self.k_cents = rs.standard_normal((M, C, dm)).astype(np.float16)
        self.v_cents = rs.standard_normal((M, C, dm)).astype(np.float16)
        self.k_codes = rs.randint(0, C, (bs, nhk, T_max, M)).astype(np.uint16)
        self.v_codes = rs.randint(0, C, (bs, nhk, T_max, M)).astype(np.uint16)
        self.k_res = rs.standard_normal((bs, nhk, cap, d)).astype(np.float16)
        self.v_res = rs.standard_normal((bs, nhk, cap, d)).astype(np.float16)
        self.k_new = rs.standard_normal((bs, nhk, 1, d)).astype(np.float16)
        self.v_new = rs.standard_normal((bs, nhk, 1, d)).astype(np.float16)
        self.T_max, self.npc = T_max, -(-T_max // ps) + 1
        self.n_pool = bs * nhk * self.npc + spare_pages
        self.ids = rs.permutation(self.n_pool)[:bs * nhk * self.npc].reshape(bs, nhk, self.npc).astype(np.int32)
        self.cents_alloc = cents_alloc
        self.upload()

    def pools(self, fill=0):
        kp = np.full((self.n_pool, self.ps, self.M), fill, np.uint16)
        vp = np.full((self.n_pool, self.M, self.ps), fill, np.uint16)
        for b in range(self.bs):
            for h in range(self.nhk):
                for pg in range(-(-self.T_max // self.ps)):
                    n = min(self.ps, self.T_max - pg * self.ps)
                    kp[self.ids[b, h, pg], :n] = self.k_codes[b, h, pg * self.ps:pg * self.ps + n]
                    vp[self.ids[b, h, pg], :, :n] = self.v_codes[b, h, pg * self.ps:pg * self.ps + n].T
        return kp, vp

    def cents_dev(self, cents):
        """The codebook on the device; cents_alloc: a view at the front of an allocation of that many entries per subspace count,
        the rest NaN (the poison test: an unmasked index reads NaN inside the allocation, never outside it)."""
        t = self.torch
        if self.cents_alloc is None:
            return t.from_numpy(cents).cuda()
        big = t.full((self.M * self.cents_alloc * cents.shape[2],), float("nan"), dtype=t.float16, device="cuda")
        view = big[:cents.size].view(*cents.shape)
        view.copy_(t.from_numpy(cents))
        return view

    def upload(self, fill=0):
        t = self.torch
        kp, vp = self.pools(fill)
        self.g = {nm: t.from_numpy(getattr(self, nm)).cuda() for nm in ("q", "k_res", "v_res", "k_new", "v_new", "ids")}
        self.g.update(k_pool=t.from_numpy(kp).cuda(), v_pool=t.from_numpy(vp).cuda(), k_cents=self.cents_dev(self.k_cents),
                      v_cents=self.cents_dev(self.v_cents))

    def run(self, ops, T, r, start=0, *, append=False, sel=slice(None), n_tokens=None, dev=None, ids=None, **kw):
        g = self.g
        if append:
            kw.update(k_new=g["k_new"][sel], v_new=g["v_new"][sel])
        return ops.pq_decode_attn_wide(g["q"][sel].contiguous(), g["k_pool"], g["v_pool"], g["k_cents"], g["v_cents"], g["k_res"][sel],
                                       g["v_res"][sel], r, n_tokens=T if n_tokens is None else n_tokens,
                                       page_ids=(g["ids"] if ids is None else ids)[sel].contiguous(), page_size=self.ps, resid_start=start,
                                       dev_lengths=dev, **kw)

    def model(self, T, r, start=0, append=False):
        return W.decode_attn(self.q, self.k_codes, self.v_codes, self.k_cents, self.v_cents, self.k_res, self.v_res, r, T=T, start=start,
                             k_new=self.k_new if append else None, v_new=self.v_new if append else None)

    def live_codes_are_wide(self, T):
        Ts = np.broadcast_to(np.asarray(T), (self.bs,))
        return all(t == 0 or (self.k_codes[b, :, :t].max() >= 256 and self.v_codes[b, :, :t].max() >= 256) for b, t in enumerate(Ts))


def within_bar(got, ref, what):
    rel, mabs = W.head_errors(got.float().cpu().numpy(), ref)
    print(f"{what}: worst head rel-L2 {rel.max():.3e}, mean-abs {mabs.max():.3e}")
    assert np.isfinite(rel).all() and rel.max() < REL_TOL and mabs.max() < MEAN_ABS_TOL, \
        f"{what}: worst head rel-L2 {rel.max():.3e} mean-abs {mabs.max():.3e} at {np.unravel_index(rel.argmax(), rel.shape)}"


def bits(t):
    return t.contiguous().view(-1).view(dtype=__import__("torch").int16).cpu().numpy()


# (d, M, C, page, G, window cap)
SHAPES = [(128, 64, 1024, 64, 4, 128), (128, 32, 4096, 128, 16, 512), (128, 64, 512, 32, 1, 64), (64, 32, 512, 64, 7, 80),
          (64, 16, 2048, 32, 16, 128)]
MAIN, M32 = SHAPES[0], SHAPES[1]


@pytest.mark.parametrize("d,M,C,ps,G,cap", SHAPES)
def test_matrix(env, d, M, C, ps, G, cap):
    torch, ops = env
    s = Store(torch, d, M, C, ps, G, cap=cap)
    n = 0
    for T in (0, 1, ps - 1, ps, ps + 1, 1029):
        for r in (0, 1, 17, cap):
            start = cap - 5 if r > 5 else (3 if r else 0)      # r = 17 and r = cap wrap around the end of the ring
            assert s.live_codes_are_wide(T)
            out, lse = s.run(ops, T, r, start, return_lse=True)
            if T == 0 and r == 0:
                assert not out.any() and torch.isneginf(lse).all()
                continue
            ref, ref_l = s.model(T, r, start)
            within_bar(out, ref, f"d{d} M{M} C{C} ps{ps} G{G} T{T} r{r}")
            assert np.abs(lse.cpu().numpy()[:, :, 0] - ref_l).max() < R.LSE_TOL
            n += 1
    assert n == 23


@pytest.mark.parametrize("d,M,C,ps,G,cap", [MAIN, SHAPES[4]])
def test_peaked_softmax_moves_the_running_maximum(env, d, M, C, ps, G, cap):
    """One key late in the context is a scaled copy of head 1's query: its score (~ 3 sqrt(d)) dwarfs every earlier one, so the
    wave that meets it moves its reference and rescales its accumulators; the other heads of the kv head do not move theirs."""
    torch, ops = env
    s = Store(torch, d, M, C, ps, G, cap=cap, seed=5)
    T, t_peak, c_peak = 1029, 1000, C - 3
    for b in range(s.bs):
        s.k_codes[b, 0, t_peak] = c_peak
    s.k_cents[:, c_peak] = (3.0 * s.q[0, 1, 0].astype(np.float32)).astype(np.float16).reshape(M, d // M)
    s.upload()
    out, lse = s.run(ops, T, 17, 100, return_lse=True)
    ref, ref_l = s.model(T, 17, 100)
    p_peak = np.exp(3.0 * (s.q[0, 1, 0].astype(np.float64) ** 2).sum() / np.sqrt(d) - ref_l[0, 1])
    assert p_peak > 0.99, p_peak
    within_bar(out, ref, f"peaked d{d} M{M} C{C}")
    assert np.abs(lse.cpu().numpy()[:, :, 0] - ref_l).max() < R.LSE_TOL


@pytest.mark.parametrize("d,M,C,ps,G,cap", [MAIN, M32])
def test_splits(env, d, M, C, ps, G, cap):
    torch, ops = env
    T = 4133
    s = Store(torch, d, M, C, ps, G, bs=1, T_max=T, cap=cap, seed=2)
    desc = ops.wide_attn_desc("test", s.g["q"], s.g["k_pool"], s.g["v_pool"], s.g["k_cents"], s.g["v_cents"], s.g["k_res"], s.g["v_res"],
                          33, T, s.g["ids"], ps, 7, None)
    assert ops.attn_wide_splits(desc) >= 2
    assert s.live_codes_are_wide(T)
    a = s.run(ops, T, 33, 7)
    b = s.run(ops, T, 33, 7)
    within_bar(a, s.model(T, 33, 7)[0], f"splits d{d} M{M} C{C}")
    assert np.array_equal(bits(a), bits(b))


def test_device_lengths(env):
    """Three requests with their own {T, r, start} rows, one of them empty, under the bound n_tokens = 1280.  The bound cuts five
    splits of 256 tokens; a request alone with host lengths T = 1029 cuts the same five, and one of 77 tokens lies in split 0 either
    way: the same tiles go to the same waves and the empty splits add exact zeros, so the bits are those of the request alone."""
    torch, ops = env
    d, M, C, ps, G, cap = MAIN
    s = Store(torch, d, M, C, ps, G, bs=3, T_max=1280, cap=cap, seed=3)
    rows = [(1029, 17, 120), (0, 0, 0), (77, cap, 50)]
    bound = 1280
    dev = torch.tensor([[T, r, st, 0] for T, r, st in rows], dtype=torch.int32, device="cuda")
    out = s.run(ops, 0, 0, 0, n_tokens=bound, dev=dev)
    assert s.live_codes_are_wide([T for T, _, _ in rows])
    ref, _ = s.model([T for T, _, _ in rows], [r for _, r, _ in rows], [st for _, _, st in rows])
    assert not out[1].any()
    for b in (0, 2):
        within_bar(out[b:b + 1], ref[b:b + 1], f"device lengths, request {b}")
    for b, (T, r, st) in enumerate(rows):
        alone = s.run(ops, T, r, st, sel=slice(b, b + 1))
        assert np.array_equal(bits(out[b]), bits(alone[0])), b
    # rows nobody should trust: T and r are clamped to the host bounds, a ring start outside the window reads as 0
    wild = torch.tensor([[-5, 2 ** 31 - 1, 9, 0], [2 ** 31 - 1, -5, cap, 0], [bound + 1, cap + 1, -1, 0]], dtype=torch.int32, device="cuda")
    tame = torch.tensor([[0, cap, 9, 0], [bound, 0, 0, 0], [bound, cap, 0, 0]], dtype=torch.int32, device="cuda")
    a = s.run(ops, 0, 0, 0, n_tokens=bound, dev=wild)
    b_ = s.run(ops, 0, 0, 0, n_tokens=bound, dev=tame)
    assert np.array_equal(bits(a), bits(b_))
    within_bar(b_, s.model([0, bound, bound], [cap, 0, cap], [9, 0, 0])[0], "clamped rows")


@pytest.mark.parametrize("use_dev", [False, True])
def test_fused_append(env, use_dev):
    torch, ops = env
    d, M, C, ps, G, cap = MAIN
    s = Store(torch, d, M, C, ps, G, cap=cap, seed=4)
    T, r, st = 333, 17, cap - 5
    row = (st + r) % cap
    before_k, before_v = s.g["k_res"].clone(), s.g["v_res"].clone()
    dev = torch.tensor([[T, r, st, 0]] * s.bs, dtype=torch.int32, device="cuda") if use_dev else None
    out, lse = s.run(ops, T, r, st, append=True, return_lse=True, **(dict(n_tokens=512, dev=dev) if use_dev else {}))
    torch.cuda.synchronize()
    assert torch.equal(s.g["k_res"][:, :, row], s.g["k_new"][:, :, 0]) and torch.equal(s.g["v_res"][:, :, row], s.g["v_new"][:, :, 0])
    keep = [i for i in range(cap) if i != row]
    assert torch.equal(s.g["k_res"][:, :, keep], before_k[:, :, keep]) and torch.equal(s.g["v_res"][:, :, keep], before_v[:, :, keep])
    if use_dev:
        assert dev.cpu().tolist() == [[T, r + 1, st, 0]] * s.bs      # incremented once
        plain = s.run(ops, 0, 0, 0, n_tokens=512, dev=dev)
        assert dev.cpu().tolist() == [[T, r + 1, st, 0]] * s.bs
    else:
        plain = s.run(ops, T, r + 1, st)
    assert np.array_equal(bits(out), bits(plain))
    ref, ref_l = s.model(T, r, st, append=True)
    within_bar(out, ref, "fused append")
    assert np.abs(lse.cpu().numpy()[:, :, 0] - ref_l).max() < R.LSE_TOL


@pytest.mark.parametrize("d,M,C,ps,G,cap", [MAIN, SHAPES[3]])
def test_lse_and_out_bits(env, d, M, C, ps, G, cap):
    torch, ops = env
    s = Store(torch, d, M, C, ps, G, cap=cap, seed=6)
    for T, r in ((1029, 17), (0, 5), (ps + 1, 0)):
        out = s.run(ops, T, r, 2)
        out2, lse = s.run(ops, T, r, 2, return_lse=True)
        buf = torch.full((s.bs, s.nh, 1), 7.0, dtype=torch.float32, device="cuda")
        out3, lse3 = s.run(ops, T, r, 2, lse=buf)
        assert lse3 is buf and np.array_equal(bits(out), bits(out2)) and np.array_equal(bits(out), bits(out3)) and torch.equal(lse, buf)
        _, ref_l = s.model(T, r, 2)
        assert np.abs(lse.cpu().numpy()[:, :, 0] - ref_l).max() < R.LSE_TOL


def test_layout_invariance(env):
    torch, ops = env
    d, M, C, ps, G, cap = SHAPES[2]
    s = Store(torch, d, M, C, ps, G, cap=cap, seed=7)
    T, r, st = 1029, 17, 60
    a = s.run(ops, T, r, st)
    b = s.run(ops, T, r, st, ids=s.g["ids"].long())
    assert np.array_equal(bits(a), bits(b))
    s.ids = np.random.RandomState(11).permutation(s.n_pool)[:s.ids.size].reshape(s.ids.shape).astype(np.int32)      # other physical pages
    s.upload()
    c = s.run(ops, T, r, st)
    assert np.array_equal(bits(a), bits(c))


@pytest.mark.parametrize("d,M,C,ps,G,cap", [MAIN, M32, SHAPES[4]])
def test_poison(env, d, M, C, ps, G, cap):
    """The same live data twice: zeros around it, then 0xFFFF codes past T in the last page and in every page no live entry names,
    table entries past the context that name such pages, NaN window rows outside the ring - bitwise the same output.  The
    codebooks are views at the front of allocations of 65536 entries per subspace whose tails are NaN: a gather without
    `& (C - 1)` reads a NaN inside the allocation and fails the comparison; it cannot read outside an allocation."""
    torch, ops = env
    T, r, st = 2 * ps + 5, 17, cap - 5
    s = Store(torch, d, M, C, ps, G, T_max=T, cap=cap, seed=8, cents_alloc=65536)
    assert s.live_codes_are_wide(T) and s.npc == 4      # three live pages, one table entry past the context
    ring = [(st + i) % cap for i in range(r)]
    dead = [i for i in range(cap) if i not in ring]
    for nm in ("k_res", "v_res"):
        getattr(s, nm)[:, :, dead] = 0
    s.upload(fill=0)
    clean, clean_l = s.run(ops, T, r, st, return_lse=True)
    within_bar(clean, s.model(T, r, st)[0], f"poison (clean) d{d} M{M} C{C}")
    for nm in ("k_res", "v_res"):
        getattr(s, nm)[:, :, dead] = np.nan
    s.upload(fill=0xFFFF)
    assert int((s.g["k_pool"].view(torch.int16) == -1).all(dim=2).all(dim=1).sum()) >= s.bs * s.nhk + 3      # pages nobody wrote, named past the context
    dirty, dirty_l = s.run(ops, T, r, st, return_lse=True)
    assert np.array_equal(bits(clean), bits(dirty)) and torch.equal(clean_l, dirty_l)
