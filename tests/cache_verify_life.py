"""Random request lifecycles with draft verification: the per-request model of tests/cache_life_model.py and its swap rules
(tests/cache_swap_life.py), by import, with one more rule

  verify_commit(n, n_draft, n_accept, route): verify moves nothing; commit appends rows 0 .. n_accept[b] - 1 of the call's K / V
      to slot b by the per-slot decode rule, n_accept[b] times, that slot only (Model.append):
          if r >= cap then T += ps, r -= ps, rs = (rs + ps) % cap; append the row, r += 1
  a refused commit (RuntimeError): nothing moves - no verify since the cache last moved (none at all, a call in between, some
      layers only), n_accept[b] > n_draft[b], a flush that would pass max_tokens

and a script generator of its own over decode bursts, prefill_request, extend_request, extend_ragged (both stores), whole and
prefix forks, release, swap_out / swap_in, verify_commit and its refusals, on all four geometries of cache_life_model - two of
them with PagedPQCache.begin_step before every decode step.  The closed form of the commit (tests/verify_model.commit_closed)
is not used here: tests/test_cache_verify_life_host.py holds the rule against it.

A verify_commit call: n, n_draft, n_accept, route ("heads", "chunk", None), reverify (every layer is verified twice, the rows
q0 / k0 / v0 first; the second set - q / k / v - is what commit takes), layers (the layers verified before the commit: all of
them, but for two of the refusals), q (layers, bs, nh, n, d), k / v (layers, bs, nh_k, n, d), NaN in every row at or past
n_draft[b].  A refused one (raises=True) names its kind in `refusal`; "moved" holds the call that runs between its verify and
its commit in `between` (a release, a fork or a decode step, applied as any call).

begin_step.  The model also keeps what the encode-ahead state of the cache depends on - one flag per slot, "the slot's oldest
page of window rows is encoded already" - and from it the kind of every decode step (Model.next_kind, PagedPQCache.next_step_kind
in the model's integers).  coverage() runs on those kinds, or on the kinds a run reports (the GPU test).

A script is every scene once - each item of REQUIRED has a scene that brings it about - in an order of the seed's, calls of no
scene in between, and last the refusal at a full page table, which needs a slot filled to max_tokens.  That makes 55 to 75
calls, at most 30 verifies, and 150 decode steps at a window of 64 rows, 230 at one of 128: a scene that wants a full window has
to pay for its rows, by decode steps (every slot's) or by rounds of 16 rows.

A seed is kept only if its script meets REQUIRED (missing()).  tests/cache_life_driver.py runs a script: for
tests/test_cache_verify_life_host.py on a CPU cache whose launches are numpy stand-ins, for tests/test_cache_verify_life_gpu.py
on a real one."""
import copy

import numpy as np

from tests import cache_life_model as LM
from tests import cache_swap_life as SL

GEOMS = LM.GEOMS
SEEDS = {"share-32": (0, 1), "share-64-ahead": (0, 320), "copy-32-ahead": (0, 2), "copy-128": (17, 18)}      # the GPU file runs the first of each
N_CALLS, MAX_ROUNDS, MAX_HELD = 50, 30, 3      # calls (about) and verify rounds (at most) per script
DECODE_BUDGET = {64: 150, 128: 230}      # decode steps per script, about, by the window's rows: a scene that needs a full window pays for one
NS = (1, 2, 4, 5, 16)      # draft rows per request; 16 rows under G = 4 query heads: 64 rows per kv head
# the refusal kinds and the word of the cache's message each must carry
REFUSALS = {"no_verify": "verify", "moved": "verify", "partial_layers": "verify", "over_accept": "n_accept", "max_tokens": "max_tokens"}


class Model(SL.Model):
    def __init__(self, geom, rows=False):
        # a window may stand behind a full page table (T = max_tokens, r <= cap): room for those rows too
        super().__init__(dict(geom, max_tokens=geom["max_tokens"] + geom["extended_residual_size"]), rows)
        self.max_tokens = geom["max_tokens"]
        self.rec = None      # the running verification: n, n_draft, (T, r, rs) when it began, the layers verified
        self.ahead, self.preallocate = geom["begin_step"], geom["preallocate"]
        self.pre = np.zeros(self.bs, bool)      # the slot's oldest page of window rows is encoded ahead
        self.ea_at = self.cap - self.ps + min(8, max(self.ps // 8, 1))      # PagedPQCache.encode_ahead_at
        self.last_kind, self.declined = None, 0

    def _put(self, b, k, v, kc, vc):
        if not self.rows:
            return
        n0, n = self.n(b), k.shape[2]
        assert n0 + n <= self.hist_k.shape[3]
        self.hist_k[:, b, :, n0:n0 + n], self.hist_v[:, b, :, n0:n0 + n] = k, v
        self.code_k[:, b, :, n0:n0 + n], self.code_v[:, b, :, n0:n0 + n] = kc, vc

    # ---- the kind of a decode step under begin_step
    def lockstep(self):
        return all((x == x[0]).all() for x in (self.T, self.r, self.rs))

    def next_kind(self):
        full = self.r >= self.cap
        if full.any():
            return "commit" if full.all() and self.pre.all() else "flush"
        if not self.pre.all() and self.r[0] >= self.ea_at and self.r[0] >= self.ps and self.lockstep():
            # a full page table has nothing to encode into: a preallocated one makes the step a plain one, paging on demand
            # refuses the page in begin_step (tests/cache_trace_scenario.py) - the generator keeps a script away from that
            room = self.T[0] + self.ps <= self.max_tokens
            assert room or self.preallocate, "begin_step would be refused here"
            return "pre" if room else "plain"
        return "plain"

    def step(self, *rows, kind=None):
        """One decode step of every slot; under begin_step of the given kind (what a run reported), or of next_kind()."""
        self.last_kind = None
        if self.ahead:
            mine = self.next_kind()
            kind = mine if kind is None else kind
            self.declined += (mine == "plain" and kind == "plain" and not (self.r >= self.cap).any() and not self.pre.all()
                              and self.r[0] >= max(self.ea_at, self.ps) and self.lockstep())
            if kind == "pre":
                self.pre[:] = True
            self.last_kind = kind
        flushed = super().step(*rows)
        self.pre[flushed] = False
        return flushed

    # ---- verify and commit
    def sig(self):
        return self.T.copy(), self.r.copy(), self.rs.copy()

    def verify(self, n, n_draft, layers):
        rec, sig = self.rec, self.sig()
        if rec is None or rec["n"] != n or rec["n_draft"] != list(n_draft) or any(not np.array_equal(a, b) for a, b in zip(rec["sig"], sig)):
            rec = self.rec = dict(n=n, n_draft=list(n_draft), sig=sig, layers=set())
        rec["layers"] |= set(layers)

    def commit_refusal(self, n_accept):
        """None, or the word of the refusal a commit of n_accept meets now."""
        rec = self.rec
        if rec is None or len(rec["layers"]) != self.nl or any(not np.array_equal(a, b) for a, b in zip(rec["sig"], self.sig())):
            return "verify"
        if len(n_accept) != self.bs or any(not 0 <= a <= nd for a, nd in zip(n_accept, rec["n_draft"])):
            return "n_accept"
        if any(a and self.r[b] + a > self.cap and self.T[b] + self.ps > self.max_tokens for b, a in enumerate(n_accept)):
            return "max_tokens"
        return None

    def append(self, b, *rows):
        """The decode rule for slot b alone; rows: k, v (layers, nh_k, 1, d) and their codes.  Returns whether the window flushed."""
        flushed = bool(self.r[b] >= self.cap)
        if flushed:
            self.T[b] += self.ps
            self.r[b] -= self.ps
            self.rs[b] = (self.rs[b] + self.ps) % self.cap
            self.pre[b] = False
        self._put(b, *rows or [None] * 4)
        self.r[b] += 1
        return flushed

    def commit(self, n_accept, *rows):
        """rows: k, v (layers, bs, nh_k, n, d) and their codes.  Returns the slots whose window flushed."""
        flushed = []
        for b, a in enumerate(n_accept):
            for i in range(a):
                if self.append(b, *[x[:, b, :, i:i + 1] for x in rows]):
                    flushed.append(b)
        return flushed

    def apply(self, call):
        op = call["op"]
        if op == "decode":
            for s in range(call["steps"]):
                self.step(*[call[key][s] for key in ("k", "v", "kc", "vc")] if self.rows else [])
            return []
        if op != "verify_commit":
            moved = super().apply(call)
            if not call.get("raises"):      # every call that joins a slot's encode-ahead clears its flag
                who = {"fork": [call.get("src")] + list(call.get("dst", ())),
                       "extend_ragged": [b for b, n in enumerate(call.get("n_new", ())) if n > 0]}.get(op, [call.get("b")])
                if op != "prefill_ragged":
                    self.pre[[b for b in who if b is not None]] = False
            return moved
        if call["layers"]:
            self.verify(call["n"], call["n_draft"], call["layers"])
        moved = self.apply(call["between"]) if call.get("between") else []
        why = self.commit_refusal(call["n_accept"])
        if call.get("raises"):
            assert why == REFUSALS[call["refusal"]], (why, call["refusal"])
            return moved
        assert why is None, why
        self.rec = None
        self.commit(call["n_accept"], *[call[key] for key in ("k", "v", "kc", "vc")] if self.rows else [])
        return [b for b, a in enumerate(call["n_accept"]) if a]


# ---------------------------------------------------------------- the coverage condition ------------------------------------
REQUIRED = dict(verify_rounds=12, commits_with_flush=3, ragged_commit_one_flushes_one_not=1, flush_commit_on_a_turned_ring=1,
                commit_lands_on_cap_next_step_flushes=1, verify_at_full_window=1, all_zero_accept_then_refused=1, partial_accept=2,
                no_draft_slot_with_tokens=1, empty_slot_started_by_commit=1, n16=1, n1=1, route_chunk=2, route_heads=2, reverify=1,
                committed_then_whole_fork=1, committed_then_prefix_fork=1, committed_then_swapped_back_and_flushed=1,
                committed_then_extend_request=1, committed_then_ragged_device_store=1, commit_on_a_restored_slot=1,
                flush_commit_with_shared_pages=1, refused_no_verify=1, refused_moved=1, refused_partial_layers=1,
                refused_over_accept=1, refused_max_tokens=1,
                # the begin_step geometries, on the kinds of their decode steps
                flush_commit_with_rows_encoded_ahead=1, commit_after_pre_then_commit_step=1, lockstep_commit_crosses_encode_ahead_at=1,
                pre_after_commit=1, commit_after_commit=1, flush_after_commit=1, plain_after_commit=1,
                encode_ahead_declined_at_a_full_table=1)
AHEAD_ONLY = ("flush_commit_with_rows_encoded_ahead", "commit_after_pre_then_commit_step", "lockstep_commit_crosses_encode_ahead_at",
              "pre_after_commit", "commit_after_commit", "flush_after_commit", "plain_after_commit", "encode_ahead_declined_at_a_full_table")


def coverage(script, geom, kinds=None):
    """The counts of REQUIRED's items in a script (and calls, decode_steps).  Pages are followed in the abstract, as LM.coverage
    does.  kinds: what begin_step answered, one entry per decode step in order (a run's report); None: Model.next_kind."""
    m, ps, cap, bs = Model(geom), geom["page_size"], geom["extended_residual_size"], geom["bs"]
    kinds = None if kinds is None else list(kinds)
    cnt = dict.fromkeys(REQUIRED, 0)
    cnt["calls"], cnt["decode_steps"] = len(script), 0
    pages, next_id = [[] for _ in range(bs)], [0]
    committed, restored, back = [False] * bs, [False] * bs, [False] * bs      # holds committed rows; swapped in; both, no flush yet
    landed, held_committed = [False] * bs, {}
    st = dict(since_commit=False, after_pre=False, zero=False)

    def grow(b):
        while len(pages[b]) * ps < m.T[b]:
            pages[b].append(next_id[0])
            next_id[0] += 1

    shared = lambda b: any(p in pages[o] for o in range(bs) if o != b for p in pages[b])

    def one_step():
        cnt["decode_steps"] += 1
        flushed = m.step(kind=kinds.pop(0) if kinds is not None and geom["begin_step"] else None)
        kind = m.last_kind
        if kind is not None and st["since_commit"]:
            cnt[kind + "_after_commit"] += 1
        cnt["commit_after_pre_then_commit_step"] += kind == "commit" and st["after_pre"]
        if flushed:
            st["after_pre"] = False
        for b in flushed:
            cnt["commit_lands_on_cap_next_step_flushes"] += landed[b]
            cnt["committed_then_swapped_back_and_flushed"] += back[b]
            back[b] = False
            grow(b)
        landed[:] = [False] * bs

    def clear(b):
        pages[b], committed[b], restored[b], back[b], landed[b] = [], False, False, False, False

    def other(call):
        op = call["op"]
        if op == "decode":
            for _ in range(call["steps"]):
                one_step()
            return
        st["since_commit"] = False
        if op == "swap_out":
            held_committed[call["snap"]] = committed[call["b"]]
            clear(call["b"])
        elif op == "swap_in":
            clear(call["b"])
            restored[call["b"]] = True
            committed[call["b"]] = back[call["b"]] = held_committed.get(call["snap"], False)
        elif op == "release":
            clear(call["b"])
        elif op == "fork":
            src, k = call["src"], call["n_tokens"]
            cnt["committed_then_whole_fork" if k is None else "committed_then_prefix_fork"] += committed[src]
            for b in call["dst"]:
                clear(b)
                pages[b] = pages[src][:(int(m.T[src]) if k is None else k) // ps]
                committed[b] = committed[src] and k is None
        elif op == "extend_request":
            cnt["committed_then_extend_request"] += committed[call["b"]]
        elif op == "extend_ragged" and call["device_store"]:
            cnt["committed_then_ragged_device_store"] += any(n > 0 and committed[b] for b, n in enumerate(call["n_new"]))
        for b in m.apply(call):
            grow(b)

    for call in script:
        zero, st["zero"] = st["zero"], False
        if call["op"] != "verify_commit":
            assert not call.get("raises")
            other(call)
            continue
        nl = geom["layer_num"]
        if call.get("raises"):
            kind, layers = call["refusal"], call["layers"]
            assert {"no_verify": not layers and not call.get("between"), "moved": len(layers) == nl and bool(call.get("between")),
                    "partial_layers": 0 < len(layers) < nl and not call.get("between")}.get(kind, len(layers) == nl and not call.get("between"))
            if call.get("between"):
                m.verify(call["n"], call["n_draft"], layers)
                other(call["between"])
                call = dict(call, layers=[], between=None)
            before = m.sig()
            m.apply(call)
            assert all(np.array_equal(a, b) for a, b in zip(before, m.sig()))
            cnt["refused_" + kind] += 1
            cnt["all_zero_accept_then_refused"] += zero and kind == "no_verify"
            continue
        assert len(call["layers"]) == nl and not call.get("between")
        nd, na = call["n_draft"], call["n_accept"]
        T0, r0, rs0 = (x.copy() for x in m.sig())
        flush = [bool(a and r0[b] + a > cap) for b, a in enumerate(na)]
        cnt["verify_rounds"] += 1
        cnt["n16"] += call["n"] == 16
        cnt["n1"] += call["n"] == 1
        cnt["route_chunk"] += call["route"] == "chunk"
        cnt["route_heads"] += call["route"] == "heads"
        cnt["reverify"] += bool(call["reverify"])
        cnt["commits_with_flush"] += any(flush)
        cnt["ragged_commit_one_flushes_one_not"] += any(flush) and any(a and not f for a, f in zip(na, flush))
        cnt["flush_commit_on_a_turned_ring"] += any(f and rs0[b] > 0 for b, f in enumerate(flush))
        cnt["flush_commit_with_shared_pages"] += any(f and shared(b) for b, f in enumerate(flush))
        cnt["verify_at_full_window"] += any(nd[b] > 0 and r0[b] == cap for b in range(bs))
        cnt["partial_accept"] += any(0 < a < d_ for a, d_ in zip(na, nd))
        cnt["no_draft_slot_with_tokens"] += any(nd[b] == 0 and T0[b] + r0[b] > 0 for b in range(bs))
        cnt["empty_slot_started_by_commit"] += any(na[b] > 0 and T0[b] + r0[b] == 0 for b in range(bs))
        cnt["commit_on_a_restored_slot"] += any(na[b] > 0 and restored[b] for b in range(bs))
        if geom["begin_step"]:
            cnt["flush_commit_with_rows_encoded_ahead"] += any(f and m.pre[b] for b, f in enumerate(flush))
            cnt["lockstep_commit_crosses_encode_ahead_at"] += (m.lockstep() and len(set(na)) == 1 and na[0] > 0 and not any(flush)
                                                               and r0[0] < m.ea_at <= r0[0] + na[0])
            if any(flush):
                st["after_pre"] = False
            elif any(na) and m.pre.all():
                st["after_pre"] = True
        for b, a in enumerate(na):
            if a:
                committed[b], restored[b] = True, False
                landed[b] = r0[b] + a == cap
        st["zero"], st["since_commit"] = not any(na), st["since_commit"] or any(na)
        for b in m.apply(call):
            grow(b)
    cnt["encode_ahead_declined_at_a_full_table"] = m.declined
    assert not kinds, "more kinds than decode steps"
    return cnt


def missing(cnt, geom):
    """{item: (have, need)} of what a script lacks.  A preallocated table shares no page; a window of one page never turns; the
    kinds of decode steps are begin_step's."""
    need = dict(REQUIRED, flush_commit_with_shared_pages=int(not geom["preallocate"]),
                flush_commit_on_a_turned_ring=int(geom["extended_residual_size"] > geom["page_size"]))
    if not geom["begin_step"]:
        need.update(dict.fromkeys(AHEAD_ONLY, 0))
    need["encode_ahead_declined_at_a_full_table"] = int(geom["begin_step"] and geom["preallocate"])
    return {k: (cnt[k], v) for k, v in need.items() if cnt[k] < v}


# ---------------------------------------------------------------- the generator ---------------------------------------------
def plan(seed, geom, rs=None):
    """The calls of a script without their rows."""
    rs = np.random.RandomState(seed) if rs is None else rs
    m, ps, cap, bs, mx, nl = Model(geom), geom["page_size"], geom["extended_residual_size"], geom["bs"], geom["max_tokens"], geom["layer_num"]
    calls, budget, rounds, next_k = [], [DECODE_BUDGET[cap]], [MAX_ROUNDS], [0]
    pick = lambda xs: xs[rs.randint(len(xs))]
    live = lambda: [b for b in range(bs) if m.n(b) > 0]
    room = lambda b: mx - m.n(b)
    others = lambda b: [int(o) for o in rs.permutation(bs) if o != b]
    can_flush = lambda b: m.T[b] + ps <= mx

    def emit(**call):
        m.apply(call)
        calls.append(call)

    def release(b):
        emit(op="release", b=int(b))

    def empty(b):
        if m.n(b) > 0:
            release(b)

    def T_after(b, steps):
        T, r = int(m.T[b]), int(m.r[b])
        for _ in range(steps):
            if r >= cap:
                T, r = T + ps, r - ps
            r += 1
        return T

    def decode(steps=None):
        if steps is None:
            steps = (1, 3, ps, cap + 3)[rs.choice(4, p=(0.35, 0.35, 0.2, 0.1))]
            if steps > budget[0] - spare_steps[0]:
                steps = pick((1, 3))
        for b in range(bs):      # a step appends to every slot: the ones whose page table has no room for their flush leave first
            if T_after(b, steps) > mx:
                release(b)
        budget[0] -= steps
        emit(op="decode", steps=int(steps))

    def prefill_request(b=None):
        b = rs.randint(bs) if b is None else b
        empty(b)
        emit(op="prefill_request", b=int(b), n=int(pick((1, ps - 1, ps, ps + 1, 3 * ps + 7))))
        return int(b)

    def a_slot(coded=False):
        ok = [b for b in live() if m.T[b] > 0 or not coded]
        return int(pick(ok)) if ok else prefill_request()

    def extend_request(b=None):
        b, n = a_slot() if b is None else b, int(pick((1, 5, ps + 3)))
        if room(b) >= n:
            emit(op="extend_request", b=b, n=n)

    def extend_ragged(must=None, device_store=None):
        n_new = [int(pick((0, 1, 5, ps, ps + 3))) for _ in range(bs)]
        n_new[rs.randint(bs)] = 0      # a slot that takes no part, always
        if must is not None:
            n_new[must] = int(pick((1, 5, ps + 3)))
        n_new = [n if room(b) >= n else 0 for b, n in enumerate(n_new)]
        if any(n_new):
            emit(op="extend_ragged", n_new=n_new, device_store=bool(rs.randint(3)) if device_store is None else device_store)

    def fork_whole(src=None, k=None):
        src = a_slot() if src is None else src
        dst = others(src)[:rs.randint(1, 3) if k is None else k]
        for b in dst:
            empty(b)
        emit(op="fork", src=src, dst=dst, n_tokens=None)
        return dst

    def fork_prefix(src=None):
        src = a_slot(coded=True) if src is None else src
        T, dst = int(m.T[src]), others(src)[0]
        empty(dst)
        emit(op="fork", src=src, dst=[dst], n_tokens=int(pick((T, T // 2, T // ps * ps, T - 1))))

    def swap_out(b=None):
        if live():
            while len(m.held) >= MAX_HELD:      # the oldest snapshot is dropped: host memory, nothing of the cache's
                del m.held[min(m.held)]
            emit(op="swap_out", b=int(pick(live())) if b is None else b, snap=next_k[0])
            next_k[0] += 1
            return next_k[0] - 1

    def swap_in(k=None, then_commit=None):
        if m.held:
            k = int(pick(sorted(m.held))) if k is None else k
            b = int(rs.randint(bs))
            empty(b)
            emit(op="swap_in", b=b, snap=k)
            if rs.randint(2) if then_commit is None else then_commit:
                commit_round(force={b: None})
            return b

    # ---- verify rounds: n, the route and reverify go round by the round's number, so that a script sees every one of them
    turn = [int(rs.randint(1000))]

    def draw(b, n, want=None):
        """(n_draft, n_accept) of slot b in a round of n rows; want: the rows the slot must accept."""
        u = rs.rand()
        nd = n if u < 0.6 else 0 if u < 0.75 else int(rs.randint(0, n + 1))
        u = rs.rand()
        a = nd if u < 0.4 else 0 if u < 0.5 else int(rs.randint(0, nd + 1))
        if want is not None:
            nd, a = max(nd, want), want
        if a and m.r[b] + a > cap and not can_flush(b):
            a = int(max(0, cap - m.r[b]))
        return nd, a

    def commit_round(n=None, force=None, zero=False):
        """One legal verify + commit.  force: {slot: rows it must accept, or None for at least one}."""
        if rounds[0] <= spare_rounds[0]:
            return False
        force = force or {}
        least = max([a or 1 for a in force.values()], default=1)
        turn[0] += 1
        if n is None:
            n = NS[turn[0] % len(NS)]
            n = n if n >= least else int(pick([x for x in NS if x >= least]))
        pairs = []
        for b in range(bs):
            nd, a = draw(b, n, force.get(b))
            if b in force and force[b] is None and a == 0:
                nd = a = n if m.r[b] + n <= cap or can_flush(b) else int(min(n, cap - m.r[b]))
            pairs.append((nd, 0 if zero else a))
        rounds[0] -= 1
        emit(op="verify_commit", n=int(n), n_draft=[p[0] for p in pairs], n_accept=[p[1] for p in pairs],
             route=("heads", "chunk", None)[turn[0] // 2 % 3], reverify=turn[0] % 6 == 0, layers=list(range(nl)))
        return True

    def fill(b, target):
        """Slot b's window to exactly `target` rows (from at most that many) by decode steps and commits; False: given up."""
        while m.r[b] < target:
            gap = int(target - m.r[b])
            by_commit = lambda: commit_round(n=16 if gap >= 16 else None, force={b: min(gap, 16)})
            if rounds[0] > spare_rounds[0] and (budget[0] - spare_steps[0] < gap or rs.rand() < 0.2):
                by_commit()
            elif budget[0] - spare_steps[0] >= gap:
                decode(gap)
            elif rounds[0] <= spare_rounds[0] or not by_commit():
                return False
            if m.n(b) == 0:
                return False
        return m.r[b] == target

    def window_at(b, target):
        """fill(), through a flush if the window is past the target already."""
        if m.r[b] > target:
            if not can_flush(b) or not fill(b, cap) or budget[0] < 1:
                return False
            decode(1)
            if m.n(b) == 0 or m.r[b] > target:
                return False
        return fill(b, target)

    def nearest(target, coded=False):
        """The live slot whose window reaches `target` rows soonest (one that can still flush)."""
        cost = lambda b: target - m.r[b] if m.r[b] <= target else cap - m.r[b] + 1 + max(0, target - (cap - ps + 1))
        ok = [b for b in live() if can_flush(b) and (m.T[b] >= ps or not coded)]
        if not ok:
            return prefill_request()
        best = min(cost(b) for b in ok)
        return int(pick([b for b in ok if cost(b) <= best + 4]))

    def land_on_cap():
        """A commit that fills the window exactly; then a verify of the full window and a flushing commit; a decode step."""
        a = int(rs.randint(1, 17))
        b = nearest(cap - a)
        if not window_at(b, cap - a) or not commit_round(force={b: a}):
            return
        if rs.randint(4) and budget[0] >= 1:
            decode(1)
        else:
            commit_round(force={b: None})
            if budget[0] >= 1:
                decode(pick((1, 3)))

    def full_window_round():
        b = nearest(cap)
        if window_at(b, cap):
            commit_round(force={b: None})

    def flush_commit(b=None, ragged=False):
        x = int(rs.randint(0, 16))
        b = nearest(cap - x) if b is None else b
        if can_flush(b) and window_at(b, cap - x):
            force = {b: int(rs.randint(cap - m.r[b] + 1, 17))}
            o = [o for o in others(b) if m.n(o) and m.r[o] + 1 <= cap]
            if ragged and o:
                force[o[0]] = int(rs.randint(1, min(16, cap - m.r[o[0]]) + 1))
            commit_round(n=16, force=force)

    def shared_flush_commit():
        src = nearest(cap - 8, coded=True)
        if m.T[src] < ps:
            if not window_at(src, cap) or budget[0] < 1:
                return
            decode(1)
            if m.n(src) == 0:
                return
        dst = fork_whole(src, k=1)
        flush_commit(int(pick([src] + dst)))

    def zero_accept():
        if commit_round(zero=True):
            refused("no_verify")

    def empty_start():
        b = int(rs.randint(bs))
        empty(b)
        commit_round(force={b: None})

    def after_commit(what):
        """A commit on a slot, then one of the calls that must go on as after decode steps."""
        b = nearest(cap - 2) if what == 2 else a_slot(coded=what == 1)
        if not commit_round(force={b: None}) or m.n(b) == 0:
            return
        if what == 0:
            fork_whole(b)
        elif what == 1 and m.T[b] > 0:
            fork_prefix(b)
        elif what == 2:
            k = swap_out(b)
            if rs.randint(2) and budget[0] >= 3:
                decode(pick((1, 3)))
            b2 = swap_in(k, then_commit=True)
            if can_flush(b2) and window_at(b2, cap) and budget[0] >= 1:
                decode(pick((1, 2)))
        elif what == 3:
            extend_request(b)
        else:
            extend_ragged(must=b, device_store=True)

    def lockstep_rounds():
        """Every slot a copy of one, then uniform commits: across encode_ahead_at(), a step that encodes ahead, on to exactly a full
        window and the step that commits the page; across encode_ahead_at() again and over the full window."""
        uniform = lambda a, n=None: commit_round(n=n, force=dict.fromkeys(range(bs), a))

        def lock_to(lo, hi):
            while m.r[0] < lo:
                glo, ghi = int(lo - m.r[0]), int(hi - m.r[0])
                steps = int(rs.randint(glo, ghi + 1))
                if budget[0] - spare_steps[0] >= steps and (rs.rand() < 0.6 or rounds[0] <= spare_rounds[0] + 3):
                    decode(steps)
                elif not uniform(16 if ghi >= 16 else int(rs.randint(glo, ghi + 1)), 16 if ghi >= 16 else None):
                    return False
            return m.lockstep() and m.n(0) > 0

        def cross():
            return uniform(int(rs.randint(m.ea_at - m.r[0], 17))) and budget[0] >= 3

        src = nearest(max(m.ea_at - 8, 0))
        if m.r[src] >= m.ea_at:
            if not fill(src, cap) or budget[0] < 1:
                return
            decode(1)
            if m.n(src) == 0:
                return
        fork_whole(src, k=bs - 1)
        if not lock_to(m.ea_at - 16, m.ea_at - 1) or not cross():
            return
        decode(pick((1, 2, 3)))      # the first one encodes ahead
        if not uniform(int(pick((5, 16))), 16) or not lock_to(cap - 16, cap - 1) or not uniform(int(cap - m.r[0])) or budget[0] < 3:
            return
        decode(pick((1, 2)))      # the windows are full and their oldest page encoded: the step commits it
        if not m.lockstep() or m.r[0] >= m.ea_at or not cross():
            return
        decode(1)
        if not lock_to(cap - 15, cap - 1):
            return
        n_acc = int(rs.randint(cap - m.r[0] + 1, 17))
        if rs.randint(2):      # one slot stays below
            commit_round(n=16, force={**dict.fromkeys(range(bs), n_acc), int(rs.randint(bs)): int(cap - m.r[0])})
        else:
            uniform(n_acc, 16)
        if budget[0] >= 1:
            decode(pick((1, 3)))

    # ---- the refusals
    def refused(kind):
        if kind != "no_verify" and not live():
            prefill_request()
        n = int(pick(NS[1:]))
        nd = [int(pick((n, n, rs.randint(0, n + 1)))) for _ in range(bs)]
        na = [int(rs.randint(0, x + 1)) if m.r[b] + x <= cap or can_flush(b) else 0 for b, x in enumerate(nd)]
        call = dict(op="verify_commit", n=n, n_draft=nd, n_accept=na, route=pick(("heads", "chunk", None)), reverify=False,
                    layers=list(range(nl)), raises=True, refusal=kind)
        if kind == "no_verify":
            call["layers"] = []
        elif kind == "partial_layers":
            call["layers"] = [int(rs.randint(nl))]
        elif kind == "over_accept":
            b = rs.randint(bs)
            nd[b] = int(rs.randint(0, n))
            na[b] = nd[b] + 1
        elif kind == "moved":
            what = rs.randint(3)
            free = [b for b in range(bs) if m.n(b) == 0]
            if what == 0 and budget[0] >= 1 and all(T_after(b, 1) <= mx for b in range(bs)):
                call["between"] = dict(op="decode", steps=1)
            elif what == 1 and free:
                call["between"] = dict(op="fork", src=int(pick(live())), dst=[int(pick(free))], n_tokens=None)
            else:
                call["between"] = dict(op="release", b=int(pick(live())))
        trial = copy.deepcopy(m)
        try:
            trial.apply(call)
        except AssertionError:      # (a verification that still stands, ...): no refusal now - after a step it is one
            if budget[0] < 1:
                return
            decode(1)
            return refused(kind)
        if kind != "no_verify":
            rounds[0] -= 1
        if call.get("between", {}).get("op") == "decode":
            budget[0] -= 1
        emit(**call)

    def refused_max_tokens():
        """A slot whose page table is full and whose window a commit would overflow; under begin_step the whole batch, in
        lockstep where the table is preallocated: its decode steps pass encode_ahead_at() with no page to encode into.  The script's last scene: what was kept
        of the decode steps and the rounds is spent here."""
        spare_steps[0] = spare_rounds[0] = 0
        b = a_slot()
        n = mx - int(pick((0, 1, ps - 1))) - m.n(b)
        if n <= 0:
            b = prefill_request(b)
            n = mx - int(pick((0, 1, ps - 1))) - m.n(b)
        emit(op="extend_request", b=b, n=int(n))
        target = cap - int(rs.randint(2, 16))
        if geom["begin_step"] and geom["preallocate"]:      # (paging on demand refuses that step)
            fork_whole(b, k=bs - 1)
            while m.r[b] < target - 8:      # in lockstep up to the last rows
                gap = int(target - 8 - m.r[b])
                if budget[0] >= gap + 9 and (rs.randint(2) or rounds[0] < 3):
                    decode(gap)
                elif rounds[0] < 2 or not commit_round(n=16 if gap >= 16 else None, force=dict.fromkeys(range(bs), min(gap, 16))):
                    return
            if budget[0] < 9:
                return
            decode(int(target - m.r[b]))
        if not fill(b, target) or budget[0] < 1 or rounds[0] < 1:
            return
        decode(1)
        nd = [16 if o == b else int(pick((0, 16))) for o in range(bs)]
        na = [16 if o == b else 0 for o in range(bs)]
        rounds[0] -= 1
        emit(op="verify_commit", n=16, n_draft=nd, n_accept=na, route=pick(("heads", "chunk", None)), reverify=False, layers=list(range(nl)),
             raises=True, refusal="max_tokens")

    # every scene once, in an order of the seed's, calls of no scene in between; the last scene is refused_max_tokens
    spare_steps, spare_rounds = [cap // 2 - 4], [cap // 32 + 2]
    fillers = [(decode, 8), (prefill_request, 4), (extend_request, 2), (extend_ragged, 4), (fork_whole, 2), (fork_prefix, 2),
               (lambda: release(rs.randint(bs)), 1), (swap_out, 3), (swap_in, 3), (commit_round, 3)]
    p = np.array([w for _, w in fillers], float)
    scenes = [zero_accept, empty_start, land_on_cap, full_window_round, lambda: flush_commit(ragged=True), flush_commit,
              lambda: refused("moved"), lambda: refused("partial_layers"), lambda: refused("over_accept")]
    scenes += [(lambda w: lambda: after_commit(w))(w) for w in range(5)]
    scenes += [shared_flush_commit] if not geom["preallocate"] else []
    scenes += [lockstep_rounds] if geom["begin_step"] else []
    prefill_request()
    decode(pick((3, ps // 2, ps)))
    for i in rs.permutation(len(scenes)):
        if rs.rand() < 0.5:
            fillers[rs.choice(len(fillers), p=p / p.sum())][0]()
        scenes[i]()
    refused_max_tokens()
    while len(calls) < N_CALLS:
        fillers[rs.choice(len(fillers), p=p / p.sum())][0]()
    return calls


def script(seed, geom, rows=True):
    return LM.script(seed, geom, rows, plan)


ROW_KEYS, encode_rows = LM.ROW_KEYS, LM.encode_rows      # (written once, for every family)
