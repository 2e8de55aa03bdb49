"""The window-length advance of a fused-append launch with device-resident lengths (csrc/attn_tail.h, "Window-length advance"):
the primary workgroup of a (request, kv head) takes the request's second-level ticket IN FRONT of its flag polls and its merge,
and the primary that took the last one bumps r - while other workgroups of the launch may still be streaming codes.  The launch
is right only if no workgroup reads its lengths after the bump, r moves exactly once per launch, and the ticket word is at rest
for the next launch, whichever kernel family that is.  The GPU tests issue step-form launches back to back, without a host
synchronisation between them, and check every launch against the fp64 oracle for ITS window (bars of
tests/test_gpu_parity.py::test_fused_append); the last test is a CPU model of the protocol over every interleaving.
"""
import ctypes

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_parity import _check

CAP, PS, START = 128, 64, 100      # window rows, tokens per page, first window row (the ring wraps: 100 + 90 > 128)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    return torch, ops


class _Steps:
    """One ragged batch in the paged layout with its lengths on the device, and the step-form launches on it."""

    def __init__(self, torch, ops, oracle, seed, bs, nh, nhk, d, M, Ts, r0s, C=256):
        from million_amd import _lib
        self.torch, self.ops, self.oracle = torch, ops, oracle
        self.bs, self.nh, self.nhk, self.d, self.M, self.C, self.Ts, self.r0s = bs, nh, nhk, d, M, C, list(Ts), list(r0s)
        self.Tmax = max(Ts)
        c = self.c = synth.attn_case(seed, bs, nh, nhk, d, M, C, self.Tmax, 0, Lt=CAP)
        self.q = torch.from_numpy(c["q"]).cuda()
        self.kp, self.vp = ops.prepare_cents(torch.from_numpy(c["k_cents"]).cuda()), ops.prepare_cents(torch.from_numpy(c["v_cents"]).cuda())
        vpool, ids = oracle.v_rowmajor_to_pool(c["v_codes"], PS)
        kpool, _ = oracle.k_rowmajor_to_pool(c["k_codes"], PS)
        self.ids = torch.from_numpy(ids.astype(np.int32)).cuda()
        self.kc, self.vc = torch.from_numpy(kpool).cuda(), torch.from_numpy(vpool).cuda()
        self.kr = torch.roll(torch.from_numpy(c["k_res"]).cuda(), START, dims=2).contiguous()
        self.vr = torch.roll(torch.from_numpy(c["v_res"]).cuda(), START, dims=2).contiguous()
        self.k_hist, self.v_hist = c["k_res"].copy(), c["v_res"].copy()      # the window in logical order (row 0 = ring row START)
        self.len0 = np.array([[Ts[b], r0s[b], START, 0] for b in range(bs)], dtype=np.int32)
        self.lengths = torch.from_numpy(self.len0).cuda()
        self.desc = ops.make_attn_desc(self.q, self.kr, nh_k=nhk, M=M, C=C, n_tokens=self.Tmax, r=0, resid_start=START, k_paged=True,
                                       v_paged=True, page_size=PS, n_pages_cap=self.ids.shape[2], dev_lengths=self.lengths)
        self.ws = torch.zeros(_lib.load().million_attn_workspace_bytes(ctypes.byref(self.desc)), dtype=torch.uint8, device="cuda")
        self.rs = np.random.RandomState(seed + 1)
        self.n = 0              # launches issued so far

    def kind(self):
        return self.ops.attn_kernel_kind(self.desc)

    def rows(self, n):
        """n new (k_new, v_new) pairs, on the device."""
        t = []
        for _ in range(n):
            k = self.rs.standard_normal((self.bs, self.nhk, 1, self.d)).astype(np.float16)
            v = self.rs.standard_normal((self.bs, self.nhk, 1, self.d)).astype(np.float16)
            t.append((k, v, self.torch.from_numpy(k).cuda(), self.torch.from_numpy(v).cuda()))
        return t

    def launch(self, row, out):
        """One step-form launch; no synchronisation."""
        self.ops.pq_decode_attn(self.q, self.kc, self.vc, self.kp, self.vp, self.kr, self.vr, 0, M=self.M, C=self.C, n_tokens=self.Tmax,
                                resid_start=START, k_page_ids=self.ids, v_page_ids=self.ids, page_size=PS, out=out,
                                dev_lengths=self.lengths, workspace=self.ws, k_new=row[2], v_new=row[3])

    def record(self, row):
        """The host's copy of what a launch did to the window."""
        for b in range(self.bs):
            self.k_hist[b, :, self.r0s[b] + self.n] = row[0][b, :, 0]
            self.v_hist[b, :, self.r0s[b] + self.n] = row[1][b, :, 0]
        self.n += 1

    def gold(self, b, k_hist, v_hist, r):
        c = self.c
        return self.oracle.decode_attn(q=c["q"][b:b + 1], k_codes=c["k_codes"][b:b + 1, :, :self.Ts[b]], v_codes=c["v_codes"][b:b + 1, :, :self.Ts[b]],
                                       k_cents=c["k_cents"], v_cents=c["v_cents"], k_res=k_hist[b:b + 1], v_res=v_hist[b:b + 1], r=r)

    def run_and_check(self, n, what, before_launch=None):
        """n launches back to back on the current stream, each with its own new rows and its own output; then every output
        against the oracle for the window as that launch saw it, the parked rows, the lengths and the fault count."""
        torch = self.torch
        rows = self.rows(n)
        outs = [torch.full_like(self.q, float("nan")) for _ in range(n)]
        torch.cuda.synchronize()
        for i in range(n):
            if before_launch:
                before_launch(i)
            self.launch(rows[i], outs[i])
        torch.cuda.synchronize()
        for i in range(n):
            self.record(rows[i])
            for b in range(self.bs):
                r = self.r0s[b] + self.n
                _check(outs[i][b:b + 1].cpu().numpy(), self.gold(b, self.k_hist, self.v_hist, r), f"{what}: launch {self.n - 1}, request {b} (T={self.Ts[b]}, r={r})")
        self.check_state(what)

    def check_state(self, what):
        got_k = self.torch.roll(self.kr, -START, dims=2).cpu().numpy()      # rows parked at (START + r0 + i) % CAP
        got_v = self.torch.roll(self.vr, -START, dims=2).cpu().numpy()
        for b in range(self.bs):
            sl = slice(self.r0s[b], self.r0s[b] + self.n)
            np.testing.assert_array_equal(got_k[b, :, sl], self.k_hist[b, :, sl], err_msg=what)
            np.testing.assert_array_equal(got_v[b, :, sl], self.v_hist[b, :, sl], err_msg=what)
        ln = self.lengths.cpu().numpy()
        assert ln[:, 1].tolist() == [r0 + self.n for r0 in self.r0s], f"{what}: r = {ln[:, 1].tolist()} after {self.n} launches from {self.r0s}"
        np.testing.assert_array_equal(ln[:, [0, 2, 3]], self.len0[:, [0, 2, 3]], err_msg=what)
        assert self.ops.tail_faults() == 0, what


@pytest.mark.gpu
@pytest.mark.parametrize("policy", [0, 16], ids=["lean", "streaming"])
@pytest.mark.parametrize("Ts,r0s", [((128, 2500), (3, 90)), ((64, 64), (3, 90))], ids=["ragged-5-splits", "single-split"])
def test_back_to_back_steps_without_host_sync(Ts, r0s, policy, env, oracle):
    """Six step-form launches on one stream with nothing between them: a workgroup that read r behind an early bump would attend to
    one row too many (and park its row one slot too far); a bump that came twice, or not at all, shows in the next launch."""
    torch, ops = env
    ops.tail_faults()
    try:
        ops.set_force_generic(policy)
        s = _Steps(torch, ops, oracle, 4200 + Ts[1] % 89, 2, 8, 2, 128, 64, Ts, r0s)
        assert s.kind() == 1
        s.run_and_check(6, f"policy {policy}")
    finally:
        ops.set_force_generic(0)


def _mfma_grid(cus, bs, nhk, T, cap):
    """Workgroups of the MFMA kernels' launch: a restatement of attn_mfma.hip's mfma_splits for contexts short of the 64-round
    limit (128 = kNW * kResRows window rows per split).  The library does not expose its plan, so this is coupled to that
    function by hand - a note beside mfma_splits says so; the two change together."""
    bh = bs * nhk
    ns = min(-(-cus // bh), 64, max(1, -(-T // 512)), max(1, -(-T // 32)))
    return bh * max(ns, 1, -(-cap // 128))


@pytest.mark.gpu
@pytest.mark.parametrize("bs", [4, 5], ids=["bs4-whole-chip", "bs5-more-than-the-chip"])
def test_steps_on_grids_that_fill_and_exceed_the_chip(bs, env, oracle):
    """32 kv heads' worth of pairs at T = 4096: three back-to-back step-form launches.  bs = 4 is 32 pairs x 8 splits = 256
    workgroups: on a 256-CU part that grid FILLS the chip but does not exceed it (the planner keeps the merge helpers at
    bh * ns <= CUs), so that shape runs with helpers; bs = 5 (40 pairs x 7 splits = 280) is the smallest batch of this shape whose
    grid exceeds the chip, where the planner sets nmerge = 1 and the ticket wave merges heads itself between request and answer -
    asserted from the planner's rule and the device's CU count."""
    torch, ops = env
    ops.tail_faults()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = _mfma_grid(cus, bs, 8, 4096, CAP)
    if bs == 5:
        assert grid > cus, f"{grid} workgroups on {cus} CUs: nmerge would not be 1"
    else:
        assert grid >= cus
    s = _Steps(torch, ops, oracle, 4300 + bs, bs, 32, 8, 128, 64, [4096] * bs, [0, 17, 64, 100, 41][:bs])
    assert s.kind() == 1
    s.run_and_check(3, f"bs={bs}")


@pytest.mark.gpu
def test_steps_with_query_head_parts(env, oracle):
    """d = 64, M = 32, 8 query heads per kv head: the lean kernel runs each kv head as two virtual kv heads of 4, AttnParams::nh_k
    is the virtual count (4) and the second-level ticket is still one word per request: r moves exactly once per launch."""
    torch, ops = env
    ops.tail_faults()
    s = _Steps(torch, ops, oracle, 4400, 2, 16, 2, 64, 32, (700, 1500), (5, 60))
    assert s.kind() == 1
    s.run_and_check(3, "query-head parts")


@pytest.mark.gpu
def test_steps_replayed_from_a_graph(env, oracle):
    """A linear graph of four step-form launches, replayed three times: r has advanced by 12 and the last replay's outputs are the
    oracle's for windows of r0 + 9 .. r0 + 12 rows more than at capture time."""
    torch, ops = env
    ops.tail_faults()
    s = _Steps(torch, ops, oracle, 4500, 2, 8, 2, 128, 64, (128, 2500), (3, 90))
    s.run_and_check(4, "eager launches in front of the capture")      # loads the kernel; also four launches of history
    rows = s.rows(4)
    outs = [torch.full_like(s.q, float("nan")) for _ in range(4)]
    r_before = s.lengths.cpu().numpy()[:, 1].copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(4):
            s.launch(rows[i], outs[i])
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert (s.lengths.cpu().numpy()[:, 1] - r_before).tolist() == [12, 12]
    for rep in range(3):
        for i in range(4):
            s.record(rows[i])
            if rep == 2:      # `outs` hold the last replay's results
                for b in range(s.bs):
                    r = s.r0s[b] + s.n
                    _check(outs[i][b:b + 1].cpu().numpy(), s.gold(b, s.k_hist, s.v_hist, r), f"replay 3, launch {i}, request {b} (r={r})")
    s.check_state("after three replays")


@pytest.mark.gpu
def test_mfma_and_tile_launches_alternate_on_one_workspace(env, oracle):
    """d = 64 on 64-token pages runs on the lean kernel, and under policy 16 on the tile kernel, whose hand-off (common.h:
    ticket_and_merge) takes the same second-level ticket word behind its merge: alternating launches of the two families on one
    workspace must each find the word at rest, agree with the oracle and move r once."""
    torch, ops = env
    ops.tail_faults()
    s = _Steps(torch, ops, oracle, 4600, 2, 8, 2, 64, 32, (300, 900), (7, 80))
    kinds = []

    def pick(i):
        ops.set_force_generic(16 if i & 1 else 0)      # read when the launch is planned, on the host
        kinds.append(s.kind())

    try:
        s.run_and_check(4, "lean / tile alternating", before_launch=pick)
    finally:
        ops.set_force_generic(0)
    assert kinds == [1, 3, 1, 3]


def _advance_model(nhk, ns, read_behind_ticket=False):
    """Every reachable state of the protocol, by exhaustive search over the interleavings of the workgroups' events (each keeps
    its own program order; the atomics on one word are serialised by the memory system, so an order of the events is all there
    is to enumerate).  A workgroup's events: 0 READ its lengths (front), 1 first-level TICKET on its pair's word (behind its
    codebook barrier, hence behind the read), and in the primary - the workgroup whose ticket completes its pair's count -
    2 the second-level ticket, taken right away, in front of its polls and its merge, 3 the ANSWER behind the merge: the primary
    that drew nh_k - 1 stores 0 to the ticket word and adds 1 to r.  read_behind_ticket swaps events 0 and 1: the order the
    kernel must never have (the negative control).  Returns (terminal states, transitions, violations)."""
    wgs = [(h, s_) for h in range(nhk) for s_ in range(ns)]
    r0 = 30
    # state: pc per workgroup, first-level counts per pair, second-level word, r, r as read per workgroup (-1: not yet), t2 per workgroup
    start = (tuple(0 for _ in wgs), tuple(0 for _ in range(nhk)), 0, r0, tuple(-1 for _ in wgs), tuple(-1 for _ in wgs))
    seen_states, todo = {start}, [start]
    terminals, transitions, violations = [], 0, []
    while todo:
        st = todo.pop()
        pc, first, cnt2, r, read, t2 = st
        moved = False
        for i, (h, _s) in enumerate(wgs):
            step = pc[i]
            if step >= 4:
                continue
            moved = True
            npc, nfirst, ncnt2, nr, nread, nt2 = list(pc), list(first), cnt2, r, list(read), list(t2)
            npc[i] = step + 1
            ev = step if not read_behind_ticket or step > 1 else 1 - step
            if ev == 0:
                nread[i] = r
            elif ev == 1:
                nfirst[h] += 1
                if first[h] != ns - 1 and step == 1:
                    npc[i] = 4                       # not the primary: nothing more
                elif first[h] != ns - 1:
                    nt2[i] = -2                      # (control order: remember it is no primary; its read is still to come)
            elif ev == 2:
                nt2[i] = cnt2
                ncnt2 = cnt2 + 1
            else:
                if t2[i] == nhk - 1:
                    if any(x < 0 for x in read):
                        violations.append("r bumped before every workgroup's length read")
                    ncnt2, nr = 0, r + 1
            if read_behind_ticket and npc[i] == 2 and nt2[i] == -2:
                npc[i] = 4
            transitions += 1
            nst = (tuple(npc), tuple(nfirst), ncnt2, nr, tuple(nread), tuple(nt2))
            if nst not in seen_states:
                seen_states.add(nst)
                todo.append(nst)
        if not moved:
            terminals.append(st)
    return terminals, transitions, violations, r0


def test_early_second_level_ticket_every_interleaving():
    """CPU model of the moved ticket (attn_tail.h, "Window-length advance"; style of tests/test_host_logic.py::
    test_split_merge_ticket_word_protocol_every_interleaving) for one request with 2 kv heads x 2 splits, and 4 x 2, 2 x 3: over
    every interleaving r is bumped exactly once, never before every workgroup's length read, every workgroup read the r of the
    launch's start, and the ticket word ends at rest.  The same search on the order the kernel must not have - a workgroup that
    takes its first-level ticket BEFORE it reads its lengths - finds the early bump: the model can tell."""
    for nhk, ns in ((2, 2), (4, 2), (2, 3), (1, 2), (2, 1)):
        terminals, transitions, violations, r0 = _advance_model(nhk, ns)
        assert not violations, (nhk, ns, violations[0])
        assert terminals and transitions > 4 * nhk * ns
        for pc, first, cnt2, r, read, t2 in terminals:
            assert r == r0 + 1, (nhk, ns, r)                       # exactly once
            assert cnt2 == 0                                        # the ticket word is at rest
            assert set(read) == {r0}                                # nobody read a bumped r
            assert list(first) == [ns] * nhk
    terminals, _, violations, r0 = _advance_model(2, 2, read_behind_ticket=True)
    assert violations and any(r0 + 1 in st[4] for st in terminals)
