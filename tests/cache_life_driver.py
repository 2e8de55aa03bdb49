"""The driver of the random request lifecycles: one script of any family (tests/cache_life_model.py, tests/cache_swap_life.py,
tests/cache_verify_life.py) on a PagedPQCache, the most derived model (cache_verify_life.Model) beside it.

What is checked, on both backends.  After every public call (a decode burst is one call; the call `between` a refused
verify_commit's verify and commit too)

  * the device lengths rows and the host mirrors are the model's integers (T, r, rs), every layer and slot;
  * the allocator's invariants hold: reference counts are the owners, no live id is free, the device table rows name the
    owners' ids, shared pages lie below every owner's T (paging on demand); the tables are as built (preallocated);
  * the encoded-ahead flags (_pre_a) are the model's, after every decode step too;
  * where the geometry says begin_step, the kind of step it reports is the model's (Model.next_kind), at every step;
  * a refused call raises RuntimeError - with the word of its refusal where the call names one - and moves nothing: the
    snapshot (cache_life_model.snapshot) after it equals the one before it.  fork, swap_in and commit are tried once,
    extend_request on every layer;
  * verify moves nothing either; swap_out's snapshot carries the model's T and ring start;
  * at the end every slot is released and nothing is left allocated or shared.

Driver is the CPU backend: a CPU cache whose launches are numpy stand-ins (stand_ins) that move the device rows the way each
call's contract says; the rows handed in are zeros, nothing reads them.  Every pool page and window row is given bytes of its
own first, and a slot restored by swap_in must hold the bytes that left at swap_out.

GpuDriver is a real cache with the script's rows, the oracle's codes of every row in the model (encode_rows), and more:

  * the codes every slot reaches through its page table are the oracle's codes of the request's own rows, byte for byte, and
    the window's ring rows are the request's last rows, bit for bit - after every call;
  * then every free pool page is filled with 0xFF (paging on demand) and every window row outside a ring span with NaN, so a
    later read of a freed page or a dead row shows as a non-finite output or a code mismatch; again between a call's verifies
    and its commit;
  * every decode step's output (every slot and layer) against oracle.decode_attn on the model's codes and window rows, every
    extend output against the fp64 chunk model of tests/test_chunk_attn_gpu.py, every prefill output against the same model
    without a past; rows past n_new[b] of a ragged call are exact zeros.  The bar is the suite's (finite, rel-L2 and mean-abs
    < 1e-3, tests/test_gpu_parity.py);
  * every layer of a verify_commit is verified with return_lse=True (twice with other rows for a `reverify` call, every set
    checked): out and lse of the rows below n_draft[b] against fp64 attention over the model's codes, window rows and the
    draft rows causally (lse_ref.chunk_ref; test_verify_gpu._check_verify: per-row rel-L2 < 1e-3, lse within lse_ref.LSE_TOL,
    finite, exact zeros and -inf at or past n_draft[b]).

A new family is a generator and a model rule of its own plus an entry in Driver.issue."""
import collections
import concurrent.futures
import contextlib
import time

import numpy as np
import pytest
import torch

from tests import cache_fork_model as FM
from tests import cache_life_model as LM
from tests import cache_swap_model as SWM
from tests import cache_verify_life as VL
from tests import store_ragged_model as SRM
from tests import verify_model as VM

REQUEST, RAGGED = ("prefill_request", "extend_request"), ("prefill_ragged", "extend_ragged")


def _same(before, after):
    return all(np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k] for k in before)


class Driver:
    """One script on a CPU cache.  run() -> self, with the kinds begin_step reported in `kinds`."""

    with_lse = False      # (the stand-ins have no log-sum-exp to give)

    def __init__(self, cache, geom, calls, rows=False):
        self.cache, self.geom, self.calls = cache, geom, calls
        self.m = VL.Model(geom, rows=rows)
        self.tables0 = cache._page_ids_all.cpu().numpy().copy()
        self.kinds, self.snaps, self.left = [], {}, {}
        self.secs = collections.Counter()      # where a script's seconds go: the host references, the snapshots and their checks

    @contextlib.contextmanager
    def clock(self, name):
        t0 = time.perf_counter()
        yield
        self.secs[name] += time.perf_counter() - t0

    # ---- what the GPU backend does otherwise
    def rows(self, call, keys=("q", "k", "v")):
        """The call's q, k, v as the script shapes them (cache_life_model.fill_rows): zeros."""
        g, op = self.geom, call["op"]
        lead = (call["steps"],) if op == "decode" else ()
        nb, n = (1, call["n"]) if op in REQUEST else (g["bs"], 1 if op == "decode" else call["n"] if op == "verify_commit" else max(call["n_new"]))
        return [torch.zeros(*lead, g["layer_num"], nb, h, n, g["d"], dtype=torch.float16) for h in (g["nh"], g["num_key_value_heads"], g["num_key_value_heads"])]

    def sync(self):
        pass

    def poison(self):
        pass

    def live(self, b):
        """The bytes slot b's request owns: its coded tokens through the page table, its window rows in ring order."""
        c = self.cache
        view16 = lambda t: t.view(torch.int16).numpy()
        T, r, st = (int(a[0, b]) for a in (c._T_a, c._r_a, c._rs_a))
        return [x.copy() for x in SWM.live_data(c._page_ids_all.numpy(), c.key_page_pool.numpy(), c.value_page_pool.numpy(),
                                                view16(c._kres_all), view16(c._vres_all), b, T, r, st)]

    def check_decode(self, call, outs, at, what):
        """outs: every (step, layer)'s output; at: (T, r) of every slot behind each step."""

    def check_chunks(self, call, outs, who, what):
        """outs: every layer's output of a prefill or an extend; who: [(index in the batch, slot, rows)]."""

    def check_verify(self, call, keys, got, what):
        """got: what verify returned for every layer of call["layers"], given the rows call[keys]."""

    def check_state(self, what):
        snap = LM.snapshot(self.cache)
        LM.check_lengths(self.m, snap, what)
        if self.geom["preallocate"]:
            LM.check_allocator_preallocated(snap, self.tables0, what)
        else:
            LM.check_allocator_on_demand(self.m, snap, what)
        return snap

    # ---- the calls
    def check_flags(self, what):
        pre = self.cache._pre_a
        assert np.array_equal(pre, np.tile(self.m.pre, (self.m.nl, 1))), f"{what}: encoded-ahead flags {pre.tolist()}, model {self.m.pre.tolist()}"

    def decode(self, call, what):
        cache, m, nl = self.cache, self.m, self.m.nl
        Q, K, V = self.rows(call)
        outs, at = [], []
        for s in range(call["steps"]):
            kind = None
            if self.geom["begin_step"]:
                want = m.next_kind()
                kind = cache.begin_step(use_dev_lengths=True)
                kind = "pre" if kind.startswith("pre") else kind
                assert kind == want, f"{what}: step {s} is a {kind!r} step, the model expects {want!r}"
                self.kinds.append(kind)
            for l in range(nl):
                outs.append(cache.decoding_with_pages(Q[s, l], K[s, l], V[s, l], l, use_dev_lengths=True).clone())
            m.step(*[call[key][s] for key in ("k", "v", "kc", "vc")] if m.rows else [], kind=kind)
            self.check_flags(f"{what}: step {s}")
            at.append((m.T.copy(), m.r.copy()))      # the rows of a burst are only appended, so every step's view stays
        self.check_decode(call, outs, at, what)

    def issue(self, call, layers, what):
        """The cache's calls of one script call (of a verify_commit the commit), with their output checks; a call that takes a
        layer is made for `layers`."""
        cache, op = self.cache, call["op"]
        if op == "release":
            cache.release(call["b"])
        elif op == "fork":
            cache.fork(call["src"], call["dst"], n_tokens=call["n_tokens"])
        elif op == "swap_out":
            b, k = call["b"], call["snap"]
            self.left[k] = self.live(b)
            self.snaps[k] = cache.swap_out(b)
            assert self.snaps[k].meta["T"] == self.m.T[b] and self.snaps[k].meta["start"] == self.m.rs[b], f"{what}: {self.snaps[k].meta}"
        elif op == "swap_in":
            cache.swap_in(call["b"], self.snaps[call["snap"]])
            for a, b in zip(self.left[call["snap"]], self.live(call["b"])):
                assert np.array_equal(a, b), f"{what}: the restored slot does not hold what left"
        elif op == "verify_commit":
            cache.commit(call["n_accept"])
        elif op in REQUEST:
            q, k, v = self.rows(call)
            outs = [getattr(cache, op)(call["b"], q[l], k[l], v[l], l) for l in layers]
            self.check_chunks(call, outs, [(0, call["b"], call["n"])], what)
        elif op in RAGGED:
            q, k, v = self.rows(call)
            outs = [getattr(cache, op)(q[l], k[l], v[l], l, call["n_new"], device_store=call["device_store"]) for l in layers]
            self.check_chunks(call, outs, [(b, b, n) for b, n in enumerate(call["n_new"]) if n], what)
        else:
            raise ValueError(op)

    def refused(self, call, what):
        self.sync()
        before = LM.snapshot(self.cache)
        for l in range(self.m.nl if call["op"] == "extend_request" else 1):      # (the other refusals are of calls that serve every layer)
            with pytest.raises(RuntimeError, match=VL.REFUSALS[call["refusal"]] if "refusal" in call else None):
                self.issue(call, [l], what)
        self.sync()
        assert _same(before, LM.snapshot(self.cache)), f"{what}: a refused call moved something"

    def verify(self, call, keys, what):
        q, k, v = self.rows(call, keys)
        got = [self.cache.verify(q[l], k[l], v[l], l, n_draft=call["n_draft"], route=call["route"], return_lse=self.with_lse) for l in call["layers"]]
        self.check_verify(call, keys, got, what)

    def do(self, call, what):
        if call["op"] == "decode":
            return self.decode(call, what)
        if call["op"] == "verify_commit":
            if call["layers"]:
                with self.clock("state checks"):
                    before = LM.snapshot(self.cache)
                if call["reverify"]:
                    self.verify(call, ("q0", "k0", "v0"), what + " (first rows)")
                self.verify(call, ("q", "k", "v"), what)
                with self.clock("state checks"):
                    assert _same(before, LM.snapshot(self.cache)), f"{what}: verify moved lengths, pages or window bytes"
            if call.get("between"):
                self.m.verify(call["n"], call["n_draft"], call["layers"])
                self.do(call["between"], what + ": between")
                self.check_state(what + ": between")
                call = dict(call, layers=[], between=None)
            self.poison()
        if call.get("raises"):
            self.refused(call, what)
        else:
            self.issue(call, range(self.m.nl), what)
        self.m.apply(call)

    def run(self):
        self.poison()
        for i, call in enumerate(self.calls):
            what = f"call {i} ({LM.describe(call)})"
            self.do(call, what)
            self.check_state(what)
            self.check_flags(what)
        self.sync()
        LM.check_end(self.cache, self.m, self.geom, self.tables0)
        return self


# ---------------------------------------------------------------- the CPU cache and its stand-ins ---------------------------
def _advance(rows, who, n, cap):
    """The flush advance of the lengths rows `who` (a mask over (rows, 4) int32), in place."""
    rows[who, 0] += n
    rows[who, 1] -= n
    rows[who, 2] = (rows[who, 2] + n) % cap


class _Nothing:
    """A stream or an event of a cache whose launches are host functions."""

    def __init__(self, *a, **k):
        pass

    wait_stream = wait_event = record = synchronize = lambda self, *a, **k: None


def stand_ins(monkeypatch):
    """numpy stand-ins of every launch the lifecycles make, and of begin_step's side stream and events (a CPU cache's launches
    run in program order)."""
    from million_amd import ops

    def decode_attn(q, *a, k_new=None, dev_lengths=None, return_lse=False, **k):
        if k_new is not None:
            dev_lengths[:, 1] += 1      # a decode step: the fused append
            return torch.zeros_like(q)
        out = torch.zeros_like(q)      # a verify launch appends nothing
        return (out, torch.zeros(q.shape[:3])) if return_lse else out

    def block_merge(q, k_blk, v_blk, out_a, lse_a, dev_n=None, out=None, lse_out=None, return_lse=False, k_stage=None, v_stage=None):
        out = torch.zeros_like(q) if out is None else out
        return (out, torch.zeros(q.shape[:3])) if return_lse else out

    def flush(k_rows, v_rows, k_cents, v_cents, k_pool, v_pool, page_ids, *, n, page_size, token_start=0, x_row_start=0,
              dev_lengths=None, min_r=0, advance=True):
        if dev_lengths is not None and advance:
            rows = dev_lengths.view(-1, 4).numpy()
            _advance(rows, rows[:, 1] >= min_r, n, k_rows.shape[-2])

    def lengths_advance(dev_lengths, n_flushed, resid_cap):
        rows = dev_lengths.numpy()
        _advance(rows, np.ones(len(rows), bool), n_flushed, resid_cap)

    def store_ragged(k_new, v_new, k_res, v_res, k_prep, v_prep, k_pool, v_pool, page_ids, dev_lengths, dev_n, *, M, C, page_size):
        dev_lengths.copy_(torch.from_numpy(SRM.advance(dev_lengths.numpy(), dev_n.numpy(), page_size=page_size, n_pages_cap=page_ids.shape[2],
                                                       resid_cap=k_res.shape[2], n_bound=k_new.shape[2])))

    def window_commit(k_new, v_new, k_res, v_res, k_prep, v_prep, k_pool, v_pool, page_ids, dev_lengths, dev_n, *, M, C, n_bound=None):
        rows, ps, cap = dev_lengths.numpy(), k_pool.shape[1], k_res.shape[3]
        assert rows.shape[:2] == (k_res.shape[0], len(dev_n)) and int(dev_n.max()) <= n_bound <= k_new.shape[3]
        for l in range(rows.shape[0]):
            for b, a in enumerate(dev_n.tolist()):
                T, r, st = VM.commit_closed(*(int(x) for x in rows[l, b, :3]), a, ps, cap)[:3]
                assert T <= page_ids.shape[3] * ps, "a flush past the page table"
                rows[l, b, :3] = (T, r, st)

    for name, f in dict(pq_encode_into=lambda *a, **k: None, prefill_attn=lambda q, k, v, **kw: torch.zeros_like(q),
                        pq_chunk_attn=lambda q, *a, **k: torch.zeros_like(q), pq_decode_attn=decode_attn, pq_flush=flush,
                        lengths_advance=lengths_advance, pq_store_ragged=store_ragged, cache_fork=FM.as_ops_stub(),
                        cache_swap=SWM.as_ops_stub(), attn_block_merge=block_merge, window_commit=window_commit,
                        decode_workspace_bytes=lambda *a, **k: 16).items():
        monkeypatch.setattr(ops, name, f)
    for name, f in dict(Stream=_Nothing, Event=_Nothing, current_stream=lambda *a, **k: _Nothing(), stream=lambda s: contextlib.nullcontext(),
                        is_current_stream_capturing=lambda: False).items():
        monkeypatch.setattr(torch.cuda, name, f)


def cpu_cache(geom):
    """As tests/cache_trace_scenario.py sets up its CPU cache: codebooks, prepared images and workspace by hand."""
    from million_amd.pq_cache import PagedPQCache
    cache = PagedPQCache(**LM.cache_kwargs(geom), device="cpu")
    cache.key_cent = cache.value_cent = torch.zeros(geom["M"], LM.C, geom["d"] // geom["M"], dtype=torch.float16)
    cache._kprep = cache._vprep = torch.zeros(1, dtype=torch.float16)
    cache._ws = torch.zeros(1, dtype=torch.uint8)
    return cache


def run_on_cpu(monkeypatch, geom, calls, seed):
    """A script (without rows) on a CPU cache under the stand-ins.  -> the driver."""
    stand_ins(monkeypatch)
    cache = cpu_cache(geom)
    # the stand-ins encode nothing: give every pool page and window row bytes of its own, so that a restored slot shows its request
    g = torch.Generator().manual_seed(seed)
    cache.key_page_pool.copy_(torch.randint(0, 256, cache.key_page_pool.shape, generator=g, dtype=torch.uint8))
    cache.value_page_pool.copy_(torch.randint(0, 256, cache.value_page_pool.shape, generator=g, dtype=torch.uint8))
    cache._kres_all.copy_(torch.randn(cache._kres_all.shape, generator=g).half())
    cache._vres_all.copy_(torch.randn(cache._vres_all.shape, generator=g).half())
    return Driver(cache, geom, calls).run()


# ---------------------------------------------------------------- the GPU ---------------------------------------------------
REL_TOL = MEAN_ABS_TOL = 1e-3      # the oracle bar of tests/test_gpu_parity.py
# the references (oracle.pq_encode, oracle.decode_attn, the chunk model) are independent pieces of C and numpy work
POOL = concurrent.futures.ThreadPoolExecutor(8)


def gpu_env():
    """The body of a GPU file's module fixture `env`: (torch, ops), and afterwards no split merge of the file's decode and
    verify launches gave up."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    yield torch, ops
    assert ops.tail_faults() == 0


class _Worst:
    """The largest errors seen, and the bar."""

    def __init__(self):
        self.rel = self.mae = 0.0
        self.n = 0

    def check(self, out, gold, what):
        out = np.asarray(out, np.float64)
        assert np.isfinite(out).all(), f"{what}: non-finite output"
        rel = np.linalg.norm(out - gold) / max(np.linalg.norm(gold), 1e-30)
        mae = np.abs(out - gold).mean()
        self.rel, self.mae, self.n = max(self.rel, rel), max(self.mae, mae), self.n + 1
        assert rel < REL_TOL and mae < MEAN_ABS_TOL, f"{what}: rel-L2 {rel:.3e} mean-abs {mae:.3e}"


def _poison(cache, m, geom):
    """0xFF in every free pool page (paging on demand), NaN in every window row outside its slot's ring span."""
    if not geom["preallocate"]:
        free = torch.tensor(sorted(cache.page_manager.free_pages), dtype=torch.long).cuda()
        cache.key_page_pool[free] = 0xFF
        cache.value_page_pool[free] = 0xFF
    dead = np.ones((m.bs, m.cap), bool)
    for b in range(m.bs):
        dead[b, (int(m.rs[b]) + np.arange(int(m.r[b]))) % m.cap] = False
    mask = torch.from_numpy(dead).cuda()[None, :, None, :].expand(m.nl, m.bs, m.nhk, m.cap)
    cache._kres_all[mask] = float("nan")
    cache._vres_all[mask] = float("nan")


class GpuDriver(Driver):
    """One script (with rows) on a real cache.  run() -> self, with `kinds`, the worst errors against the oracle in `worst`, the
    worst verify row error and the number of verified (layer, slot) blocks in `ver`, and `secs`."""

    with_lse = True

    def __init__(self, oracle, geom, calls):
        from million_amd.pq_cache import PagedPQCache
        from tests.test_chunk_attn_gpu import model
        from tests.test_verify_gpu import _check_verify
        self.oracle, self.chunk_model, self._check_verify = oracle, model, _check_verify
        self.ck, self.cv = ck, cv = LM.codebooks(geom)
        oracle.lib()
        t0 = time.perf_counter()
        LM.encode_rows(calls, geom, lambda x: oracle.pq_encode(x, ck), lambda x: oracle.pq_encode(x, cv), POOL)
        encode_s = time.perf_counter() - t0
        cache = PagedPQCache(**LM.cache_kwargs(geom), device="cuda")
        cache.set_cent(self.dev(ck), self.dev(cv))
        super().__init__(cache, geom, calls, rows=True)
        self.secs["oracle codes"] = encode_s
        self.worst, self.ver = _Worst(), dict(rel=0.0, n=0)

    @staticmethod
    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def rows(self, call, keys=("q", "k", "v")):
        return [self.dev(call[key]) for key in keys]

    def sync(self):
        torch.cuda.synchronize()

    def poison(self):
        _poison(self.cache, self.m, self.geom)

    def live(self, b):
        return []      # (check_state reads every slot's codes and window rows, a restored one's too)

    def check_state(self, what):
        torch.cuda.synchronize()
        with self.clock("state checks"):
            snap = super().check_state(what)
            LM.check_codes(self.m, snap, what)
            LM.check_window(self.m, snap, what)
            self.poison()

    def check_decode(self, call, outs, at, what):
        m, g, ck, cv = self.m, self.geom, self.ck, self.cv
        torch.cuda.synchronize()
        got = torch.stack(outs).float().cpu().numpy().reshape(call["steps"], m.nl, m.bs, g["nh"], 1, g["d"])

        def gold(key):
            s, l, b = key
            T, r = int(at[s][0][b]), int(at[s][1][b])
            return self.oracle.decode_attn(call["q"][s, l, b:b + 1], *m.codes(l, b, T), ck, cv, *m.window(l, b, T, r), r)
        keys = [(s, l, b) for s in range(call["steps"]) for l in range(m.nl) for b in range(m.bs)]
        with self.clock("references"):
            golds = list(POOL.map(gold, keys))
        for (s, l, b), gd in zip(keys, golds):
            self.worst.check(got[s, l, b:b + 1], gd, f"{what}: step {s} layer {l} slot {b} (T={at[s][0][b]} r={at[s][1][b]})")

    def check_chunks(self, call, outs, who, what):
        """fp64 outputs of the chunks q / k / v (layers, slots, heads, n, d) of the slots `who` over what each slot holds now."""
        m, g, ck, cv = self.m, self.geom, self.ck, self.cv
        q, k, v = call["q"], call["k"], call["v"]
        torch.cuda.synchronize()

        def gold(l, j, b, n):
            (kc, vc), (kw, vw) = m.codes(l, b), m.window(l, b)
            return self.chunk_model(self.oracle, q[l][j:j + 1, :, :n], kc, vc, ck, cv, kw, vw, k[l][j:j + 1, :, :n], v[l][j:j + 1, :, :n])
        keys = [(l, j, b, n) for l in range(m.nl) for j, b, n in who]
        with self.clock("references"):
            golds = {key[:2]: gd for key, gd in zip(keys, POOL.map(lambda key: gold(*key), keys))}
        n_rows = call["n"] if call["op"] in REQUEST else max(call["n_new"])
        counts = {j: n for j, _, n in who}
        for l in range(m.nl):
            out = outs[l].float().cpu().numpy()
            assert out.shape == (q.shape[1], g["nh"], n_rows, g["d"])
            for j in range(q.shape[1]):
                n = counts.get(j, 0)
                assert not out[j, :, n:].any(), f"{what}: layer {l} slot {j}: rows past n_new={n} are not zeros"
            for j, b, n in who:
                self.worst.check(out[j:j + 1, :, :n], golds[l, j], f"{what}: layer {l} slot {b} (T={m.T[b]} r={m.r[b]})")

    def check_verify(self, call, keys, got, what):
        """Every layer's out and lse against fp64 over what the model holds."""
        from tests import lse_ref as R
        m, g, ck, cv = self.m, self.geom, self.ck, self.cv
        q, k, v = (call[key] for key in keys)
        nd = call["n_draft"]
        torch.cuda.synchronize()

        def ref(key):
            l, b = key
            if nd[b] == 0:      # no row to compare: zeros and -inf are asked of the output itself
                return np.zeros((1,) + q[l].shape[1:]), np.full((1,) + q[l].shape[1:3], -np.inf)
            (kc, vc), (kw, vw) = m.codes(l, b), m.window(l, b)
            st = dict(q=q[l][b:b + 1], k_res=kw, k_codes=kc, v_codes=vc, k_cents=ck, v_cents=cv, k_win=kw, v_win=vw,
                      k_ch=k[l][b:b + 1], v_ch=v[l][b:b + 1])
            return R.chunk_ref(self.oracle, st, [nd[b]])
        pairs = [(l, b) for l in call["layers"] for b in range(m.bs)]
        with self.clock("references"):
            refs = dict(zip(pairs, POOL.map(ref, pairs)))
        for l, gl in zip(call["layers"], got):
            assert gl[0].shape == (m.bs, g["nh"], call["n"], g["d"]) and gl[1].shape == (m.bs, g["nh"], call["n"])
            ro, rl = (np.concatenate([refs[l, b][i] for b in range(m.bs)]) for i in range(2))
            self.ver["rel"] = max(self.ver["rel"], self._check_verify(gl, (ro, rl), nd, f"{what}: verify of layer {l} (T={m.T.tolist()} r={m.r.tolist()})"))
            self.ver["n"] += sum(x > 0 for x in nd)
