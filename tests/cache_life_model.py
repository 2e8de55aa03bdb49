"""Random request lifecycles of a PagedPQCache against a per-request model: the model, the script generator, the coverage
condition, the row filler of every family of scripts and the invariant checks.  tests/cache_life_driver.py runs a script on a
cache and says what is checked; tests/test_cache_life_host.py (CPU cache, launches replaced by numpy stand-ins) and
tests/test_cache_life_gpu.py (real cache, real bits) name the scripts.  numpy only (snapshot() copies a cache's tensors to the
host).

The model.  Per slot b and layer: the fp16 K and V rows the request was given, in order, with the oracle's codes of every row
(oracle.pq_encode, once per row - encode_rows: a code depends on nothing but its row and the codebook), and three integers T, r, rs -
the first T rows are codes behind the slot's page table, the next r are the window, ring rows (rs + i) % cap.  T + r is the
number of rows, always.  The rules:

  prefill_request(b, n), prefill_ragged (slots with n_new[b] > 0, which must be empty): the n rows; T = n, r = rs = 0
  decode step (every slot, idle ones too): if r >= cap then T += ps, r -= ps, rs = (rs + ps) % cap; append the row, r += 1
  extend_request(b, n), extend_ragged (slots with n_new[b] > 0): append the n rows; T += r + n, r = rs = 0
  fork(src, dsts): every destination becomes a copy of the source
  fork(src, dst, n_tokens=k): the source's first k rows; T = k, r = rs = 0
  release(b): empty, zeros
  a refused call (RuntimeError): nothing moves

A script is a list of calls (dicts) with their row data; script(seed, geom) draws both from np.random.RandomState(seed).
SEEDS names the scripts the tests run: a seed is kept only if its script meets REQUIRED (coverage)."""
import numpy as np

BASE = dict(bs=4, nh=8, num_key_value_heads=2, layer_num=2, d=128, max_tokens=1024)
C = 256
# the smallest geometries at which each path exists.  begin_step: PagedPQCache.begin_step(use_dev_lengths=True) before every
# decode step (encode-ahead).  copy-128: the window is one page, every flush empties it.
GEOMS = {
    "share-32": dict(BASE, preallocate=False, page_size=32, extended_residual_size=64, M=64, begin_step=False),
    "share-64-ahead": dict(BASE, preallocate=False, page_size=64, extended_residual_size=128, M=64, begin_step=True),
    "copy-32-ahead": dict(BASE, preallocate=True, page_size=32, extended_residual_size=64, M=32, begin_step=True),
    "copy-128": dict(BASE, preallocate=True, page_size=128, extended_residual_size=128, M=64, begin_step=False),
}
SEEDS = {"share-32": (28, 60), "share-64-ahead": (87, 121), "copy-32-ahead": (17, 20), "copy-128": (11, 25)}
N_CALLS, DECODE_BUDGET = 80, 300      # calls per script (a decode burst is one call); decode steps per script, about


def cache_kwargs(geom):
    """The constructor arguments of PagedPQCache among a geometry's entries."""
    return {k: v for k, v in geom.items() if k != "begin_step"}


def codebooks(geom):
    """(key, value) codebooks (M, C, d / M) fp16, built as tests/test_cache_fork_gpu.py builds them."""
    from tests import synth
    nhk, d, M = geom["num_key_value_heads"], geom["d"], geom["M"]
    return synth.encode_case(4400, 1, nhk, 1, d, M, C)["cents"], synth.encode_case(4401, 1, nhk, 1, d, M, C)["cents"]


# ---------------------------------------------------------------- the model ------------------------------------------------
class Model:
    """rows = False: the three integers per slot only (generator, coverage, the CPU test); else the rows and their codes too
    (the calls carry both: encode_rows)."""

    def __init__(self, geom, rows=False):
        self.bs, self.nl, self.nhk, self.d = geom["bs"], geom["layer_num"], geom["num_key_value_heads"], geom["d"]
        self.ps, self.cap, self.max_tokens = geom["page_size"], geom["extended_residual_size"], geom["max_tokens"]
        self.T, self.r, self.rs = (np.zeros(self.bs, np.int64) for _ in range(3))
        self.rows = rows
        if rows:
            rows = (self.nl, self.bs, self.nhk, self.max_tokens, self.d)
            self.hist_k, self.hist_v = np.zeros(rows, np.float16), np.zeros(rows, np.float16)
            self.code_k, self.code_v = (np.zeros(rows[:4] + (geom["M"],), np.uint8) for _ in range(2))

    def n(self, b):
        return int(self.T[b] + self.r[b])

    def _put(self, b, k, v, kc, vc):
        """k, v (layers, nh_k, n, d) with their codes kc, vc (layers, nh_k, n, M): the slot's next rows.  Before the integers move."""
        if not self.rows:
            return
        n0, n = self.n(b), k.shape[2]
        assert n0 + n <= self.max_tokens
        self.hist_k[:, b, :, n0:n0 + n], self.hist_v[:, b, :, n0:n0 + n] = k, v
        self.code_k[:, b, :, n0:n0 + n], self.code_v[:, b, :, n0:n0 + n] = kc, vc

    def prefill(self, b, n, *rows):
        assert self.n(b) == 0
        self._put(b, *rows or [None] * 4)
        self.T[b], self.r[b], self.rs[b] = n, 0, 0

    def step(self, *rows):
        """One decode step; rows: k, v (layers, bs, nh_k, 1, d) and their codes.  Returns the slots whose window flushed."""
        flushed = [b for b in range(self.bs) if self.r[b] >= self.cap]
        for b in flushed:
            self.T[b] += self.ps
            self.r[b] -= self.ps
            self.rs[b] = (self.rs[b] + self.ps) % self.cap
        for b in range(self.bs):
            self._put(b, *[a[:, b] for a in rows] or [None] * 4)
            self.r[b] += 1
        return flushed

    def extend(self, b, n, *rows):
        self._put(b, *rows or [None] * 4)
        self.T[b], self.r[b], self.rs[b] = self.n(b) + n, 0, 0

    def fork(self, src, dsts, n_tokens=None):
        for b in dsts:
            assert self.n(b) == 0 and b != src
            if self.rows:
                for a in (self.hist_k, self.hist_v, self.code_k, self.code_v):
                    a[:, b] = a[:, src]
            if n_tokens is None:
                self.T[b], self.r[b], self.rs[b] = self.T[src], self.r[src], self.rs[src]
            else:
                assert 0 <= n_tokens <= self.T[src]
                self.T[b], self.r[b], self.rs[b] = n_tokens, 0, 0

    def release(self, b):
        self.T[b] = self.r[b] = self.rs[b] = 0

    # what the checks and the attention references read
    def codes(self, l, b, T=None):
        """K and V codes of the slot's T coded tokens, (1, nh_k, T, M).  (T, and r below: the slot at an earlier moment of a
        decode burst - a burst only appends rows.)"""
        T = int(self.T[b] if T is None else T)
        return self.code_k[l, b:b + 1, :, :T], self.code_v[l, b:b + 1, :, :T]

    def window(self, l, b, T=None, r=None):
        """K and V window rows in ring order, (1, nh_k, r, d)."""
        T, r = int(self.T[b] if T is None else T), int(self.r[b] if r is None else r)
        return self.hist_k[l, b:b + 1, :, T:T + r], self.hist_v[l, b:b + 1, :, T:T + r]

    def refuses(self, call):
        """Whether the cache must refuse the call (the two refusals the scripts hold)."""
        if call["op"] == "fork":
            return any(self.n(b) > 0 for b in call["dst"])
        if call["op"] == "extend_request":
            return self.n(call["b"]) + call["n"] > self.max_tokens
        return False

    def apply(self, call):
        """Every call but a decode burst (step by step: the callers look at each step).  Returns the slots that took rows."""
        op = call["op"]
        if call.get("raises"):
            assert self.refuses(call), call["op"]
            return []
        assert not self.refuses(call)
        rows = lambda b, n, one: [call[key][:, 0 if one else b, :, :n] for key in ("k", "v", "kc", "vc")] if self.rows else []
        if op == "prefill_request":
            self.prefill(call["b"], call["n"], *rows(call["b"], call["n"], True))
        elif op == "extend_request":
            self.extend(call["b"], call["n"], *rows(call["b"], call["n"], True))
        elif op in ("prefill_ragged", "extend_ragged"):
            for b, n in enumerate(call["n_new"]):
                if n > 0:
                    (self.prefill if op == "prefill_ragged" else self.extend)(b, n, *rows(b, n, False))
            return [b for b, n in enumerate(call["n_new"]) if n > 0]
        elif op == "fork":
            self.fork(call["src"], call["dst"], call["n_tokens"])
            return list(call["dst"])
        elif op == "release":
            self.release(call["b"])
        else:
            raise ValueError(op)
        return [call["b"]]


# ---------------------------------------------------------------- the coverage condition ------------------------------------
REQUIRED = dict(whole_forks=3, whole_forks_multi=1, prefix_forks=2, prefix_page_multiple=1, prefix_inside_a_page=1,
                grandchild_flush_after_origin_release=1, source_released_then_prefill_request=1, flush_with_shared_pages=1,
                ragged_device_store_forked_and_idle=2, ragged_host_store=1, prefill_ragged_device_store=1,
                prefill_ragged_host_store=1, refused_fork=1, refused_extend=1,
                whole_fork_of_a_turned_ring=1)      # a window that starts inside the ring (where the window is more than one page)


def coverage(script, geom):
    """The counts of REQUIRED's items in a script (and calls, decode_steps).  Pages are followed in the abstract - one id per
    page of a slot's coded tokens, a fork handing the source's full pages to its destinations - whatever the geometry."""
    m, ps, bs = Model(geom), geom["page_size"], geom["bs"]
    cnt = dict.fromkeys(REQUIRED, 0)
    cnt["calls"], cnt["decode_steps"] = len(script), 0
    life, parent, grand, freed_src = [0] * bs, [None] * bs, [None] * bs, [False] * bs
    pages, next_id = [[] for _ in range(bs)], [0]

    def grow(b):
        while len(pages[b]) * ps < m.T[b]:
            pages[b].append(next_id[0])
            next_id[0] += 1

    shared = lambda b: any(p in pages[o] for o in range(bs) if o != b for p in pages[b])
    for call in script:
        op = call["op"]
        if call.get("raises"):
            assert m.refuses(call)
            cnt["refused_fork" if op == "fork" else "refused_extend"] += 1
            continue
        if op == "decode":
            for _ in range(call["steps"]):
                cnt["decode_steps"] += 1
                for b in m.step():
                    cnt["flush_with_shared_pages"] += shared(b)
                    if grand[b] is not None:      # the grandchild's first flush: its origin must be gone by now
                        cnt["grandchild_flush_after_origin_release"] += life[grand[b][0]] != grand[b][1]
                        grand[b] = None
                    grow(b)
            freed_src = [False] * bs
            continue
        if op == "release":
            b = call["b"]
            freed_src[b] = any(parent[o] == (b, life[b]) and m.n(o) > 0 for o in range(bs))
            life[b] += 1
            parent[b] = grand[b] = None
            pages[b] = []
        elif op == "fork":
            src, k = call["src"], call["n_tokens"]
            if k is None:
                cnt["whole_forks"] += 1
                cnt["whole_forks_multi"] += len(call["dst"]) >= 2
                cnt["whole_fork_of_a_turned_ring"] += m.r[src] > 0 and m.rs[src] > 0
            else:
                cnt["prefix_forks"] += 1
                cnt["prefix_page_multiple"] += k > 0 and k % ps == 0
                cnt["prefix_inside_a_page"] += k % ps != 0
            full, tail = divmod(int(m.T[src]) if k is None else k, ps)
            for b in call["dst"]:
                pages[b] = pages[src][:full]
                if (m.n(src) if k is None else k) > 0:
                    parent[b] = (src, life[src])
                    grand[b] = parent[src]
        elif op == "prefill_request":
            cnt["source_released_then_prefill_request"] += freed_src[call["b"]]
        elif op == "prefill_ragged":
            cnt["prefill_ragged_device_store" if call["device_store"] else "prefill_ragged_host_store"] += 1
        elif op == "extend_ragged":
            if not call["device_store"]:
                cnt["ragged_host_store"] += 1
            elif 0 in call["n_new"] and any(n > 0 and parent[b] is not None for b, n in enumerate(call["n_new"])):
                cnt["ragged_device_store_forked_and_idle"] += 1
        for b in m.apply(call):
            grow(b)
            if op != "release":
                freed_src[b] = False
    return cnt


def missing(cnt, geom):
    """{item: (have, need)} of what a script lacks.  A window of one page never turns: its ring start stays 0."""
    need = dict(REQUIRED, whole_fork_of_a_turned_ring=int(geom["extended_residual_size"] > geom["page_size"]))
    return {k: (cnt[k], v) for k, v in need.items() if cnt[k] < v}


# ---------------------------------------------------------------- the generator ---------------------------------------------
def plan(seed, geom, rs=None):
    """The calls of a script without their rows."""
    rs = np.random.RandomState(seed) if rs is None else rs
    m, ps, cap, bs, mx = Model(geom), geom["page_size"], geom["extended_residual_size"], geom["bs"], geom["max_tokens"]
    calls, budget = [], [DECODE_BUDGET]
    pick = lambda xs: xs[rs.randint(len(xs))]
    live = lambda: [b for b in range(bs) if m.n(b) > 0]
    room = lambda b: mx - m.n(b)
    others = lambda b: [int(o) for o in rs.permutation(bs) if o != b]

    def emit(**call):
        if call["op"] == "decode":
            for _ in range(call["steps"]):
                m.step()
        else:
            m.apply(call)
        calls.append(call)

    def release(b):
        emit(op="release", b=int(b))

    def empty(b):
        if m.n(b) > 0:
            release(b)

    def decode(steps=None):
        if steps is None:
            steps = (1, 3, ps, cap + 3)[rs.choice(4, p=(0.35, 0.35, 0.15, 0.15))]
        if steps > budget[0]:
            steps = pick((1, 3))
        for b in range(bs):      # a step appends to every slot: the ones without the room leave first
            if room(b) < steps:
                release(b)
        budget[0] -= steps
        emit(op="decode", steps=int(steps))

    def prefill_request(b=None):
        b = rs.randint(bs) if b is None else b
        empty(b)
        emit(op="prefill_request", b=int(b), n=int(pick((1, ps - 1, ps, ps + 1, 3 * ps + 7))))

    def a_source(coded=False):
        ok = [b for b in live() if m.T[b] > 0 or not coded]
        if not ok:
            prefill_request()
            ok = [b for b in live() if m.T[b] > 0]
        return int(pick(ok))

    def prefill_ragged():
        who = others(-1)[:rs.randint(1, bs)]
        for b in who:
            empty(b)
        n_new = [0] * bs
        for b in who:
            n_new[b] = int(pick((1, ps - 1, ps, ps + 1, 3 * ps + 7)))
        if len(who) > 1 and rs.randint(4) == 0:
            n_new[who[0]] = 0      # an empty slot that takes no part
        emit(op="prefill_ragged", n_new=n_new, device_store=bool(rs.randint(2)))

    def extend_request():
        b, n = rs.randint(bs), pick((1, 5, ps, ps + 3))
        if room(b) < n:
            release(b)
        emit(op="extend_request", b=int(b), n=int(n))

    def extend_ragged():
        n_new = [int(pick((0, 1, 5, ps, ps + 3))) for _ in range(bs)]
        n_new = [n if room(b) >= n else 0 for b, n in enumerate(n_new)]
        n_new[rs.randint(bs)] = 0      # a slot that takes no part, always
        if not any(n_new):
            n_new[pick([b for b in range(bs) if room(b) >= 1] or [0])] = 1
        if all(room(b) >= n for b, n in enumerate(n_new)):
            emit(op="extend_ragged", n_new=n_new, device_store=bool(rs.randint(3)))

    def fork_whole(k=None, src=None):
        src = a_source() if src is None else src
        dst = others(src)[:rs.randint(1, bs) if k is None else k]
        for b in dst:
            empty(b)
        emit(op="fork", src=src, dst=dst, n_tokens=None)
        return dst

    def fork_prefix(src=None, dst=None):
        src = a_source(coded=True) if src is None else src
        T = int(m.T[src])
        dst = others(src)[0] if dst is None else dst
        empty(dst)
        emit(op="fork", src=src, dst=[dst], n_tokens=int(pick((0, T, T // 2, T // ps * ps, T - 1))))

    def fork_all():
        """Every slot a copy of one: the batch is in lockstep, so the steps behind it can encode ahead and commit."""
        if budget[0] >= cap + 3:
            fork_whole(k=bs - 1)
            decode(cap + 3)

    def family():
        """A -> B -> C; A leaves while both live and a new request takes its slot; everybody crosses a flush."""
        if budget[0] < cap + 6:
            return
        a = a_source(coded=True)
        b, c = others(a)[:2]
        empty(b)
        emit(op="fork", src=a, dst=[b], n_tokens=None)
        if rs.randint(2) and min(room(x) for x in range(bs)) >= 3:
            decode(pick((1, 3)))
        if rs.randint(2) and m.T[b] > 0:
            fork_prefix(src=b, dst=c)
        else:
            empty(c)
            emit(op="fork", src=b, dst=[c], n_tokens=None)
        release(a)
        prefill_request(a)
        decode(cap + 3)

    def refused_fork():
        if len(live()) >= 2:
            src = a_source()
            emit(op="fork", src=src, dst=[int(pick([b for b in live() if b != src]))], n_tokens=None, raises=True)

    def refused_extend():
        if live():
            b = int(max(live(), key=m.n))
            emit(op="extend_request", b=b, n=int(room(b) + 1), raises=True)

    moves = [(decode, 26), (extend_request, 8), (extend_ragged, 16), (prefill_request, 6), (prefill_ragged, 9), (fork_whole, 8),
             (fork_prefix, 9), (fork_all, 4), (family, 5), (lambda: release(rs.randint(bs)), 3), (refused_fork, 3), (refused_extend, 3)]
    p = np.array([w for _, w in moves], float)
    while len(calls) < N_CALLS:
        moves[rs.choice(len(moves), p=p / p.sum())][0]()
    return calls


def fill_rows(calls, geom, rs):
    """The rows of every call, standard-normal fp16 drawn from rs in the calls' order: decode bursts q (steps, layers, bs, nh, 1, d),
    k / v (steps, layers, bs, nh_k, 1, d); one request q (layers, 1, nh, n, d), k / v (layers, 1, nh_k, n, d); ragged batches and
    verify_commit calls (tests/cache_verify_life.py) q (layers, bs, nh, n, d), k / v alike, n = max n_new or the call's, NaN in the
    rows past n_new[b] or n_draft[b] (they may hold anything); a `reverify` call a second set after the first, q0 / k0 / v0; then
    the rows of the call in `between`."""
    nl, bs, nh, nhk, d = geom["layer_num"], geom["bs"], geom["nh"], geom["num_key_value_heads"], geom["d"]
    f = lambda *s: rs.standard_normal(s).astype(np.float16)

    def fill(call):
        op = call["op"]
        if op == "decode":
            call["q"], call["k"], call["v"] = f(call["steps"], nl, bs, nh, 1, d), f(call["steps"], nl, bs, nhk, 1, d), f(call["steps"], nl, bs, nhk, 1, d)
        elif op in ("prefill_request", "extend_request"):
            call["q"], call["k"], call["v"] = f(nl, 1, nh, call["n"], d), f(nl, 1, nhk, call["n"], d), f(nl, 1, nhk, call["n"], d)
        elif op in ("prefill_ragged", "extend_ragged", "verify_commit"):
            n, counts = (call["n"], call["n_draft"]) if op == "verify_commit" else (max(call["n_new"]), call["n_new"])
            for keys in (("q", "k", "v"), ("q0", "k0", "v0"))[:2 if call.get("reverify") else 1]:
                call[keys[0]], call[keys[1]], call[keys[2]] = f(nl, bs, nh, n, d), f(nl, bs, nhk, n, d), f(nl, bs, nhk, n, d)
                for b, nb in enumerate(counts):
                    for key in keys:
                        call[key][:, b, :, nb:] = np.nan
            if call.get("between"):
                fill(call["between"])
    for call in calls:
        fill(call)
    return calls


def script(seed, geom, rows=True, plan=plan):
    """The calls of plan(seed, geom), with their rows (fill_rows), all from RandomState(seed).  (plan: the generator of another
    family of scripts - tests/cache_swap_life.py, tests/cache_verify_life.py.)"""
    rs = np.random.RandomState(seed)
    calls = plan(seed, geom, rs)
    return fill_rows(calls, geom, rs) if rows else calls


def encode_rows(calls, geom, f_k, f_v, pool):
    """call["kc"], call["vc"]: the codes of every row a script hands to the model, shaped as the rows with M in the last axis -
    each row's codes computed once, by f_k / f_v ((1, 1, n, d) fp16 -> (1, 1, n, M) uint8: oracle.pq_encode with the key / value
    codebook), on the threads of `pool` (a concurrent.futures executor; the oracle's C loops run without the interpreter lock).
    Of a ragged batch the rows below n_new[b], of a verify_commit those below n_accept[b] (the model takes no other); a refused
    call's rows are nobody's, but for the decode step between its verify and its commit."""
    tasks = []

    def add(call):
        if call.get("between"):
            add(call["between"])
        if "k" not in call or call.get("raises"):
            return
        counts = call["n_accept"] if call["op"] == "verify_commit" else call.get("n_new")
        for key, f in (("k", f_k), ("v", f_v)):
            x = call[key]
            out = call[key + "c"] = np.zeros(x.shape[:-1] + (geom["M"],), np.uint8)
            if counts is not None:
                tasks.extend((f, x[:, b, :, :n], out[:, b, :, :n]) for b, n in enumerate(counts) if n)
            else:
                tasks.append((f, x, out))
    for call in calls:
        add(call)

    def run(task):
        f, x, out = task
        out[...] = f(np.ascontiguousarray(x).reshape(1, 1, -1, x.shape[-1])).reshape(out.shape)
    list(pool.map(run, tasks))


# ---------------------------------------------------------------- what a cache holds, as plain arrays ------------------------
def snapshot(cache):
    """Device rows, tables, pools and windows on the host, the mirrors and the allocator's state (copies)."""
    host = lambda t: t.cpu().numpy().copy()
    pm = cache.page_manager
    import torch
    return dict(lengths=host(cache._lengths_all), T_a=cache._T_a.copy(), r_a=cache._r_a.copy(), rs_a=cache._rs_a.copy(),
                page_ids=host(cache._page_ids_all), k_pool=host(cache.key_page_pool), v_pool=host(cache.value_page_pool),
                k_res=host(cache._kres_all.view(torch.int16)), v_res=host(cache._vres_all.view(torch.int16)),
                host_pids=[[[list(h) for h in b] for b in l] for l in cache._host_pids],
                ref={pid: pm.ref_count(pid) for pid in pm.allocated_pages}, free=set(pm.free_pages),
                allocated_pages=pm.get_stats()["allocated_pages"], sharing=cache.sharing_stats())


# ---------------------------------------------------------------- the invariants -------------------------------------------
def check_lengths(m, snap, what=""):
    """The device rows' first three words and the host mirrors are the model's (T, r, rs), every layer and slot."""
    want = np.stack([m.T, m.r, m.rs], axis=1)
    for l in range(m.nl):
        got = snap["lengths"][l, :, :3]
        assert np.array_equal(got, want), f"{what}: device lengths of layer {l} {got.tolist()}, model {want.tolist()}"
        mirror = np.stack([snap["T_a"][l], snap["r_a"][l], snap["rs_a"][l]], axis=1)
        assert np.array_equal(mirror, want), f"{what}: host mirror of layer {l} {mirror.tolist()}, model {want.tolist()}"


def gather_codes(snap, l, b, T, ps):
    """K and V codes (nh_k, T, M) of a slot's first T tokens through its device table row (V pages are transposed)."""
    n = -(-T // ps)
    ids = snap["page_ids"][l, b, :, :n].astype(np.int64)
    assert ids.min() >= 0 and ids.max() < snap["k_pool"].shape[0], f"page ids outside the pool: {ids.tolist()}"
    k = snap["k_pool"][ids]
    v = snap["v_pool"][ids].transpose(0, 1, 3, 2)
    return k.reshape(k.shape[0], n * ps, -1)[:, :T], v.reshape(v.shape[0], n * ps, -1)[:, :T]


def check_codes(m, snap, what=""):
    """Every slot's T coded tokens, reached through its page table, are the oracle's codes of its first T rows."""
    for l in range(m.nl):
        for b in range(m.bs):
            T = int(m.T[b])
            if T == 0:
                continue
            for side, got, want in zip("KV", gather_codes(snap, l, b, T, m.ps), m.codes(l, b)):
                if not np.array_equal(got, want[0]):
                    bad = np.argwhere(got != want[0])
                    toks = np.unique(bad[:, 1])
                    raise AssertionError(f"{what}: {side} codes of layer {l} slot {b} (T={T}) differ from the model at {len(toks)} tokens, "
                                         f"first token {toks[0]} (page {toks[0] // m.ps}), last {toks[-1]}")


def check_window(m, snap, what=""):
    """Ring rows (rs + i) % cap, i < r, are the slot's rows T .. T + r, bit for bit."""
    for l in range(m.nl):
        for b in range(m.bs):
            ring = (int(m.rs[b]) + np.arange(int(m.r[b]))) % m.cap
            for side, got, want in zip("KV", (snap["k_res"], snap["v_res"]), m.window(l, b)):
                got = got[l, b][:, ring]
                if not np.array_equal(got, want[0].view(np.int16)):
                    rows = np.unique(np.argwhere(got != want[0].view(np.int16))[:, 1])
                    raise AssertionError(f"{what}: {side} window of layer {l} slot {b} (T={m.T[b]} r={m.r[b]} rs={m.rs[b]}) differs from "
                                         f"the model at window rows {rows[:8].tolist()}")


def check_allocator_on_demand(m, snap, what=""):
    """Paging on demand: reference counts are the owners, no live id is free, the device rows name the owners' ids, a page
    with more than one owner lies wholly below every owner's T."""
    owners = {}
    for l, layer in enumerate(snap["host_pids"]):
        for b, slot in enumerate(layer):
            for h, ids in enumerate(slot):
                assert len(set(ids)) == len(ids), f"{what}: layer {l} slot {b} head {h} names a page twice: {ids}"
                assert len(ids) * m.ps >= m.T[b], f"{what}: layer {l} slot {b} head {h}: {len(ids)} pages for T={m.T[b]}"
                row = snap["page_ids"][l, b, h, :len(ids)].tolist()
                assert row == ids, f"{what}: device table row of layer {l} slot {b} head {h} is {row}, the host's list {ids}"
                for j, pid in enumerate(ids):
                    owners.setdefault(pid, []).append((l, b, h, j))
    for pid in set(owners) | set(snap["ref"]):
        assert snap["ref"].get(pid, 0) == len(owners.get(pid, ())), (f"{what}: page {pid} has reference count {snap['ref'].get(pid, 0)} "
                                                                      f"and owners {owners.get(pid, [])}")
    assert not set(owners) & snap["free"], f"{what}: live pages on the free list: {sorted(set(owners) & snap['free'])}"
    assert snap["allocated_pages"] == len(owners), f"{what}: {snap['allocated_pages']} pages allocated, {len(owners)} live"
    for pid, own in owners.items():
        if len(own) > 1:
            for l, b, h, j in own:
                assert (j + 1) * m.ps <= m.T[b], (f"{what}: page {pid} has {len(own)} owners and is page {j} of layer {l} slot {b} head {h}, "
                                                 f"whose T={m.T[b]} ends inside it")
    want = {"shared_pages": sum(len(o) > 1 for o in owners.values()), "extra_references": sum(len(o) - 1 for o in owners.values())}
    assert snap["sharing"] == want, f"{what}: sharing_stats {snap['sharing']}, the owners give {want}"


def check_allocator_preallocated(snap, tables0, what=""):
    """A preallocated table: distinct ids, as built."""
    assert np.unique(snap["page_ids"]).size == snap["page_ids"].size, f"{what}: a preallocated table names a page twice"
    assert np.array_equal(snap["page_ids"], tables0), f"{what}: a preallocated table changed"
    assert snap["sharing"] == {"shared_pages": 0, "extra_references": 0}, f"{what}: {snap['sharing']}"


def check_end(cache, m, geom, tables0):
    """Every slot released: nothing is left allocated (on demand), nothing shared, every length zero."""
    for b in range(m.bs):
        cache.release(b)
        m.release(b)
    snap = snapshot(cache)
    check_lengths(m, snap, "end of script")
    assert not snap["lengths"].any(), snap["lengths"].tolist()
    assert snap["sharing"] == {"shared_pages": 0, "extra_references": 0}
    if geom["preallocate"]:
        check_allocator_preallocated(snap, tables0, "end of script")
    else:
        check_allocator_on_demand(m, snap, "end of script")
        assert snap["allocated_pages"] == 0 and not snap["ref"] and len(snap["free"]) == cache.page_manager.current_active_pages


ROW_KEYS = ("q", "k", "v", "kc", "vc", "q0", "k0", "v0")


def describe(call):
    """A call without its rows, for messages."""
    return ", ".join(f"{k}=({describe(v)})" if k == "between" and v else f"{k}={v}" for k, v in call.items() if k not in ROW_KEYS)
