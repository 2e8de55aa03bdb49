"""Random request lifecycles with swaps: the per-request model and the invariant checks of tests/cache_life_model.py, by
import, with two more rules

  swap_out(b) -> k : the slot becomes empty (as release); the model keeps the request - its rows, their codes, T, r, rs - as
                     snapshot k
  swap_in(b, k)    : the empty slot b becomes the request of the held snapshot k (which stays held: a snapshot is a copy)
  a refused swap_in (the slot holds tokens): nothing moves

and a script generator of its own over the calls decode, prefill_request, extend_request, fork (whole), release, swap_out and
swap_in.  A seed is kept only if its script meets REQUIRED (a swap of a slot with shared pages is asked of the
on-demand geometry only - a preallocated table shares nothing - so on the GPU share-32 / seed 37 is the script that has one).
tests/cache_life_driver.py runs a script: for tests/test_cache_swap_life_host.py on a CPU cache whose launches are numpy
stand-ins, for tests/test_cache_swap_life_gpu.py on a real one."""
import numpy as np

from tests import cache_life_model as LM

GEOMS = {"share-32": LM.GEOMS["share-32"], "copy-128": LM.GEOMS["copy-128"]}      # one on demand, one preallocated; no begin_step
SEEDS = {"share-32": (37, 18), "copy-128": (23, 17)}      # the GPU file runs the first of each
N_CALLS, DECODE_BUDGET, MAX_HELD = 45, 260, 3


class Model(LM.Model):
    def __init__(self, geom, rows=False):
        super().__init__(geom, rows)
        self.held = {}

    def swap_out(self, b, k):
        snap = dict(T=int(self.T[b]), r=int(self.r[b]), rs=int(self.rs[b]), slot=b)
        if self.rows:
            snap["rows"] = [a[:, b].copy() for a in (self.hist_k, self.hist_v, self.code_k, self.code_v)]
        self.held[k] = snap
        self.release(b)

    def swap_in(self, b, k):
        snap = self.held[k]
        assert self.n(b) == 0
        if self.rows:
            for a, saved in zip((self.hist_k, self.hist_v, self.code_k, self.code_v), snap["rows"]):
                a[:, b] = saved
        self.T[b], self.r[b], self.rs[b] = snap["T"], snap["r"], snap["rs"]

    def refuses(self, call):
        if call["op"] == "swap_in":
            return self.n(call["b"]) > 0
        return super().refuses(call)

    def apply(self, call):
        if call["op"] == "swap_out":
            self.swap_out(call["b"], call["snap"])
            return [call["b"]]
        if call["op"] == "swap_in":
            if call.get("raises"):
                assert self.refuses(call)
                return []
            assert not self.refuses(call)
            self.swap_in(call["b"], call["snap"])
            return [call["b"]]
        return super().apply(call)


# ---------------------------------------------------------------- the coverage condition ------------------------------------
REQUIRED = dict(swap_outs=3, swap_ins=3, swap_out_with_shared_pages=1, swap_in_into_another_slot=1, swap_in_after_source_reused=1,
                refused_swap_in=1, swap_of_a_turned_ring=1, flush_after_swap_in=1, whole_forks=1)


def coverage(script, geom):
    """The counts of REQUIRED's items in a script.  Pages are followed in the abstract, as LM.coverage does."""
    m, ps, bs = Model(geom), geom["page_size"], geom["bs"]
    cnt = dict.fromkeys(REQUIRED, 0)
    cnt["calls"], cnt["decode_steps"] = len(script), 0
    pages, next_id, restored, reused = [[] for _ in range(bs)], [0], [False] * bs, {}

    def grow(b):
        while len(pages[b]) * ps < m.T[b]:
            pages[b].append(next_id[0])
            next_id[0] += 1

    def new_request(b):
        for k, snap in m.held.items():
            if snap["slot"] == b:
                reused[k] = True

    shared = lambda b: any(p in pages[o] for o in range(bs) if o != b for p in pages[b])
    for call in script:
        op = call["op"]
        if call.get("raises"):
            assert m.refuses(call)
            cnt["refused_swap_in"] += op == "swap_in"
            continue
        if op == "decode":
            for _ in range(call["steps"]):
                cnt["decode_steps"] += 1
                for b in m.step():
                    cnt["flush_after_swap_in"] += restored[b]
                    restored[b] = False
                    grow(b)
            continue
        if op == "swap_out":
            cnt["swap_outs"] += 1
            cnt["swap_out_with_shared_pages"] += shared(call["b"])
            cnt["swap_of_a_turned_ring"] += m.r[call["b"]] > 0 and m.rs[call["b"]] > 0
            pages[call["b"]], restored[call["b"]] = [], False
        elif op == "swap_in":
            cnt["swap_ins"] += 1
            cnt["swap_in_into_another_slot"] += m.held[call["snap"]]["slot"] != call["b"]
            cnt["swap_in_after_source_reused"] += reused.get(call["snap"], False)
            new_request(call["b"])
            pages[call["b"]], restored[call["b"]] = [], True
        elif op == "release":
            pages[call["b"]], restored[call["b"]] = [], False
        elif op == "fork":
            cnt["whole_forks"] += 1
            for b in call["dst"]:
                new_request(b)
                pages[b], restored[b] = pages[call["src"]][:int(m.T[call["src"]]) // ps], False
        elif op == "prefill_request":
            new_request(call["b"])
        for b in m.apply(call):
            grow(b)
    return cnt


def missing(cnt, geom):
    """{item: (have, need)} of what a script lacks.  A preallocated table shares no page; a window of one page never turns."""
    need = dict(REQUIRED, swap_out_with_shared_pages=int(not geom["preallocate"]),
                swap_of_a_turned_ring=int(geom["extended_residual_size"] > geom["page_size"]))
    return {k: (cnt[k], v) for k, v in need.items() if cnt[k] < v}


# ---------------------------------------------------------------- the generator ---------------------------------------------
def plan(seed, geom, rs=None):
    """The calls of a script without their rows."""
    rs = np.random.RandomState(seed) if rs is None else rs
    m, ps, cap, bs, mx = Model(geom), geom["page_size"], geom["extended_residual_size"], geom["bs"], geom["max_tokens"]
    calls, budget, next_k = [], [DECODE_BUDGET], [0]
    pick = lambda xs: xs[rs.randint(len(xs))]
    live = lambda: [b for b in range(bs) if m.n(b) > 0]
    room = lambda b: mx - m.n(b)

    def emit(**call):
        if call["op"] == "decode":
            for _ in range(call["steps"]):
                m.step()
        else:
            m.apply(call)
        calls.append(call)

    def empty(b):
        if m.n(b) > 0:
            emit(op="release", b=int(b))

    def decode():
        steps = (1, 3, ps, cap + 3)[rs.choice(4, p=(0.3, 0.3, 0.2, 0.2))]
        if steps > budget[0]:
            steps = pick((1, 3))
        for b in range(bs):      # a step appends to every slot: the ones without the room leave first
            if room(b) < steps:
                emit(op="release", b=b)
        budget[0] -= steps
        emit(op="decode", steps=int(steps))

    def prefill_request():
        b = rs.randint(bs)
        empty(b)
        emit(op="prefill_request", b=int(b), n=int(pick((1, ps - 1, ps, ps + 1, 3 * ps + 7))))

    def extend_request():
        if live():
            b, n = int(pick(live())), int(pick((1, 5, ps + 3)))
            if room(b) >= n:
                emit(op="extend_request", b=b, n=n)

    def fork():
        if not live():
            return prefill_request()
        src = int(pick(live()))
        dst = [int(o) for o in rs.permutation(bs) if o != src][:rs.randint(1, 3)]
        for b in dst:
            empty(b)
        emit(op="fork", src=src, dst=dst, n_tokens=None)

    def swap_out():
        if live():
            while len(m.held) >= MAX_HELD:      # the oldest snapshot is dropped: host memory, nothing of the cache's
                del m.held[min(m.held)]
            emit(op="swap_out", b=int(pick(live())), snap=next_k[0])
            next_k[0] += 1

    def swap_in():
        if m.held:
            k = int(pick(sorted(m.held)))
            b = int(rs.randint(bs))
            empty(b)
            emit(op="swap_in", b=b, snap=k)

    def refused_swap_in():
        if m.held and live():
            emit(op="swap_in", b=int(pick(live())), snap=int(pick(sorted(m.held))), raises=True)

    moves = [(decode, 28), (prefill_request, 10), (extend_request, 8), (fork, 12), (lambda: empty(rs.randint(bs)), 4), (swap_out, 16),
             (swap_in, 16), (refused_swap_in, 4)]
    p = np.array([w for _, w in moves], float)
    while len(calls) < N_CALLS:
        moves[rs.choice(len(moves), p=p / p.sum())][0]()
    return calls


def script(seed, geom, rows=True):
    return LM.script(seed, geom, rows, plan)
