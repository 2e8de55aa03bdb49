"""One scripted life of a CPU PagedPQCache with every launch replaced by a recorder: the host bookkeeping as a trace.

run(preallocate) walks prefill, ~100 decode steps per layer (in-line flushes with host and with device lengths), commits,
extend, release / prefill_request, extend_request, the ragged forms, update, the hipGraph mirror calls and every rejection,
and after each public call records the `ops` calls it made (name, scalars, tensor dtype / shape / storage offset, the values
of small int32 tensors), the six mirror arrays, the device length rows, the page tables and the PageManager counters.
compact() keeps of each record only what differs from the record before (and of each ops call only the arguments that differ
from the same call one public call of that label earlier, or else from the last call of that name), which is what tests/cache_trace.json holds and tests/test_cache_transitions.py compares.

The committed trace was written by the bookkeeping as it stood before the mirror transitions got one owner each; it is the
definition of "behaviour unchanged" for pq_cache.py.  `python -m tests.cache_trace_scenario` rewrites it: only for a change
that is MEANT to move the bookkeeping, and then the diff of the JSON is the review.
"""
import json
from pathlib import Path

import torch

TRACE = Path(__file__).with_name("cache_trace.json")
OPS = ("pq_encode_into", "pq_flush", "pq_chunk_attn", "pq_decode_attn", "prefill_attn", "lengths_advance")
GEOM = dict(bs=3, nh=8, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=32, extended_residual_size=64, max_tokens=1024)
_DT = {torch.float16: "f16", torch.uint8: "u8", torch.int32: "i32", torch.float32: "f32", torch.int64: "i64"}


def _enc(v):
    if isinstance(v, torch.Tensor):
        s = f"{_DT[v.dtype]}{list(v.shape)}@{v.storage_offset()}"
        return s + (f"={v.tolist()}" if v.dtype == torch.int32 and v.numel() <= 32 else "")
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, (list, tuple)):
        return [_enc(x) for x in v]
    raise TypeError(f"unrecorded argument type {type(v)}")


class Life:
    def __init__(self, preallocate):
        from million_amd import ops
        from million_amd.pq_cache import PagedPQCache
        self.ops, self.cls, self.preallocate = ops, PagedPQCache, preallocate
        self.calls, self.records = [], []
        self.saved = {name: getattr(ops, name) for name in OPS}

    def __enter__(self):
        def recorder(name):
            def f(*a, **k):
                self.calls.append((name, {**{str(i): _enc(x) for i, x in enumerate(a)}, **{n: _enc(x) for n, x in k.items()}}))
                return torch.zeros_like(a[0]) if name in ("pq_chunk_attn", "pq_decode_attn", "prefill_attn") else None
            return f
        for name in OPS:
            setattr(self.ops, name, recorder(name))
        return self

    def __exit__(self, *exc):
        for name, f in self.saved.items():
            setattr(self.ops, name, f)

    def cache(self):
        c = self.cls(**GEOM, preallocate=self.preallocate, device="cpu")
        c.key_cent = c.value_cent = torch.zeros(64, 256, 2, dtype=torch.float16)
        c._kprep = c._vprep = torch.zeros(1, dtype=torch.float16)
        c._ws = torch.zeros(1, dtype=torch.uint8)      # the decode workspace is sized through the library: not here
        self.c = c
        self.note("new cache")
        return c

    def note(self, label, raised=None):
        c = self.c
        st = {"pm": list(c.page_manager.get_stats().values())}
        for l in range(c.layer_num):
            for name, arr in (("T", c._T_a), ("r", c._r_a), ("rs", c._rs_a), ("seen", c._seen_a), ("pre", c._pre_a),
                              ("pages", c._pages_a), ("len", c.lengths)):
                row = arr[l].tolist()
                st[f"{name}{l}"] = row[0] if name != "len" and row == row[:1] * c.bs else row      # one value: every request's
            for b in range(c.bs):      # a request's page table, each kv head's row without its trailing zeros
                st[f"pids{l}.{b}"] = [row[:max([i + 1 for i, x in enumerate(row) if x], default=0)] for row in c.page_ids[l][b].tolist()]
        self.records.append({"call": label, "raised": raised, "ops": self.calls, "state": st})
        self.calls = []

    @staticmethod
    def label(name, a, k):
        show = lambda x: "x".join(map(str, x.shape)) if isinstance(x, torch.Tensor) else str(x)
        return f"{name}({', '.join([show(x) for x in a] + [f'{n}={show(x)}' for n, x in k.items()])})"

    def do(self, name, *a, **k):
        """c.<name>(*a, **k), recorded; the tensors of the call appear in the label by shape."""
        label = self.label(name, a, k)
        out = getattr(self.c, name)(*a, **k)
        self.note(label)
        return out

    def rejects(self, name, *a, **k):
        label = self.label(name, a, k)
        try:
            getattr(self.c, name)(*a, **k)
        except (RuntimeError, ValueError) as e:
            self.note(label, raised=f"{type(e).__name__}: {e}")
            return
        raise AssertionError(f"{label} did not raise")


def _q(bs, n):
    return torch.zeros(bs, GEOM["nh"], n, GEOM["d"], dtype=torch.float16)


def _x(bs, n):
    return torch.zeros(bs, GEOM["num_key_value_heads"], n, GEOM["d"], dtype=torch.float16)


def _decode(life, steps, use_dl, begin=False):
    for _ in range(steps):
        if begin:
            life.do("begin_step", use_dev_lengths=use_dl)
        for l in range(GEOM["layer_num"]):
            life.do("decoding_with_pages", _q(3, 1), _x(3, 1), _x(3, 1), l, use_dev_lengths=use_dl)


def run(preallocate):
    """The records of one life: [{"call", "raised", "ops": [(name, {argument: value})], "state": {...}}]."""
    L_, cap, ps = GEOM["layer_num"], GEOM["extended_residual_size"], GEOM["page_size"]
    with Life(preallocate) as life:
        c = life.cache()
        # 1. lockstep prefill (a prompt that does not end on a page)
        for l in range(L_):
            life.do("prefill", _q(3, 40), _x(3, 40), _x(3, 40), l)
        # 2. decode: in-line flushes at steps 65 (host lengths) and 97 (device lengths)
        _decode(life, 70, False)
        _decode(life, 30, True)
        # direct flush calls: below a page nothing moves; page_size <= r < cap moves with host lengths only
        c.set_host_state((c._seen_a, [ps - 1] * L_, c._T_a, c._rs_a))
        life.do("flush_to_pages", 0)
        c.set_host_state((c._seen_a, [ps + 5] * L_, c._T_a, c._rs_a))
        life.do("flush_to_pages", 0, use_dev_lengths=True)
        life.do("flush_to_pages", 0)
        life.do("flush_to_pages", 1)
        # 3. commit at a full window with the flags set, host lengths and device lengths; the steps around it
        for use_dl in (False, True):
            c.set_host_state((c._seen_a, [cap] * L_, c._T_a, c._rs_a, [1] * L_))
            life.do("next_step_kind")
            _decode(life, 2, use_dl, begin=True)
        # 4. extend: a wrapped window and a chunk, every request
        c.set_host_state((c._seen_a, [40] * L_, c._T_a, [50] * L_, [1, 0]))
        for l in range(L_):
            c._sync_lengths(l)
            life.do("extend", _q(3, 10), _x(3, 10), _x(3, 10), l)
        # 5. one slot recycled
        life.do("release", 1)
        for l in range(L_):
            life.do("prefill_request", 1, _q(1, 45), _x(1, 45), _x(1, 45), l)
        # requests at different lengths: device lengths serve them, only full windows flush
        _decode(life, 3, True)
        c._r_a[:, 1] = cap
        c._pre_a[:] = 1
        life.do("next_step_kind")
        life.do("flush_to_pages", 0, use_dev_lengths=True)
        _decode(life, 2, True)
        # 6. extend_request: a slot with a window, an empty slot
        for l in range(L_):
            life.do("extend_request", 1, _q(1, 5), _x(1, 5), _x(1, 5), l)
        life.do("release", 2)
        life.do("extend_request", 2, _q(1, 9), _x(1, 9), _x(1, 9), 0)
        # 7. the ragged forms, one idle slot each
        life.do("release", 0)
        life.do("release", 2)
        for l in range(L_):
            life.do("prefill_ragged", _q(3, 33), _x(3, 33), _x(3, 33), l, [33, 0, 17])
        _decode(life, 4, True)
        for l in range(L_):
            life.do("extend_ragged", _q(3, 12), _x(3, 12), _x(3, 12), l, [12, 0, 7])
        life.do("release", 1)
        life.do("extend_ragged", _q(3, 6), _x(3, 6), _x(3, 6), 0, [0, 6, 3])      # an empty slot rides along
        life.do("get_cache_stats")
        life.do("cleanup")

        # 8. update on a fresh cache
        c = life.cache()
        c._codes_rowmajor = lambda l, T: (torch.zeros(3, 2, T, 64, dtype=torch.uint8),) * 2
        saved, life.ops.pq_decode = life.ops.pq_decode, lambda codes, cents: torch.zeros(*codes.shape[:3], 128, dtype=torch.float16)
        try:
            for n, distort in ((20, False), (13, False), (8, True)):
                life.do("update", _x(3, n), _x(3, n), 0, distort_recent=distort)
        finally:
            life.ops.pq_decode = saved

        # 9. the mirror of a captured step: one state per kind, one replayed step of each
        c = life.cache()
        for groups in (None, 2):
            c.encode_ahead_steps = groups
            c.set_host_state(([96] * L_, [0] * L_, [96] * L_, [32] * L_))
            for kind, state in life.do("capture_states"):
                c.set_host_state(state)
                life.do("host_state")
                life.do("next_step_kind")
                life.do("note_replayed_step", kind)
        c.encode_ahead_steps = None
        c.set_host_state(([96] * L_, [[63, cap, 10], [cap, cap, cap]], [[96, 64, 0], [96, 96, 96]], [[0, 32, 0], [32, 32, 32]], [1] * L_))
        life.do("note_replayed_step")
        life.do("note_replayed_step")
        # an encode-ahead step with no room left encodes nothing
        c.set_host_state(([1040] * L_, [40] * L_, [1000] * L_, [0] * L_))
        life.do("next_step_kind")
        (life.do if preallocate else life.rejects)("begin_step")      # on-demand: the page past the capacity is refused
        life.do("note_replayed_step", "pre")

        # 10. every rejection: the message, no launch, nothing moved
        c = life.cache()
        life.rejects("prefill", _q(3, 1100), _x(3, 1100), _x(3, 1100), 0)
        c._T_a[0] = [64, 32, 0]
        c._r_a[1] = [5, 0, 0]
        life.rejects("prefill", _q(3, 4), _x(3, 4), _x(3, 4), 0)
        life.rejects("prefill_request", 0, _q(1, 4), _x(1, 4), _x(1, 4), 0)
        life.rejects("prefill_request", 0, _q(1, 4), _x(1, 4), _x(1, 4), 1)
        life.rejects("prefill_request", 2, _q(3, 4), _x(3, 4), _x(3, 4), 0)
        life.rejects("prefill_request", 2, _q(1, 1100), _x(1, 1100), _x(1, 1100), 0)
        life.rejects("prefill_ragged", _q(3, 8), _x(3, 8), _x(3, 8), 0, [8, 8])
        life.rejects("prefill_ragged", _q(3, 8), _x(3, 8), _x(3, 7), 0, [8, 0, 0])
        life.rejects("prefill_ragged", _q(3, 8), _x(3, 8), _x(3, 8), 0, [0, 0, 9])
        life.rejects("prefill_ragged", _q(3, 8), _x(3, 8), _x(3, 8), 0, [0, -1, 0])
        life.rejects("prefill_ragged", _q(3, 8), _x(3, 8), _x(3, 8), 0, [0, 3, 8])
        life.rejects("prefill_ragged", _q(3, 1100), _x(3, 1100), _x(3, 1100), 0, [0, 0, 1100])
        life.rejects("extend", _q(3, 4), _x(3, 4), _x(3, 4), 0)
        life.rejects("extend", _q(3, 4), _x(3, 4), _x(3, 4), 1)
        life.rejects("extend_request", 0, _q(3, 4), _x(3, 4), _x(3, 4), 0)
        life.rejects("extend_request", 0, _q(1, 1000), _x(1, 1000), _x(1, 1000), 0)
        life.rejects("extend_ragged", _q(3, 8), _x(3, 8), _x(3, 8), 0, [8, 8])
        life.rejects("extend_ragged", _q(3, 8), _x(3, 8), _x(3, 8), 0, [9, 0, 0])
        life.rejects("extend_ragged", _q(3, 8), _x(3, 8), _x(3, 8), 0, [0, -2, 0])
        life.rejects("extend_ragged", _q(3, 1000), _x(3, 1000), _x(3, 1000), 0, [1000, 0, 5])
        life.rejects("update", _x(3, 4), _x(3, 4), 0)
        life.rejects("update", _x(3, 4), _x(3, 4), 1)
        life.rejects("decoding_with_pages", _q(3, 1), _x(3, 1), _x(3, 1), 0)
        c._r_a[0] = [cap, 0, cap]
        life.rejects("flush_to_pages", 0)
        life.rejects("decoding_with_pages", _q(3, 1), _x(3, 1), _x(3, 1), 0)
        c._T_a[0, 2] = 1000
        life.rejects("flush_to_pages", 0, use_dev_lengths=True)
        c.set_host_state(([1064] * L_, [cap] * L_, [1000] * L_, [0] * L_))
        life.rejects("flush_to_pages", 1)
        life.rejects("extend", _q(3, 4), _x(3, 4), _x(3, 4), 1)
        return life.records


def _delta(prev, cur):
    return {k: v for k, v in cur.items() if k not in prev or prev[k] != v}


def compact(records):
    """Lossless and small: the labels once, in a table; of each record's state only what differs from the record before; of
    each ops call only the arguments that differ from the same call of the previous public call with this label (or else
    from the last call of that name)."""
    labels, rows, state, last = [], [], {}, {}
    for rec in records:
        if rec["call"] not in labels:
            labels.append(rec["call"])
        calls = []
        for i, (name, args) in enumerate(rec["ops"]):
            calls.append([name, _delta(last.get((rec["call"], i, name), last.get(name, {})), args)])
            last[rec["call"], i, name] = last[name] = args
        rows.append([labels.index(rec["call"]), calls, _delta(state, rec["state"])] + ([rec["raised"]] if rec["raised"] else []))
        state = rec["state"]
    return {"labels": labels, "records": rows}


def first_difference(got, want):
    """Where two compact traces part, in words (for the assertion message)."""
    if got["labels"] != want["labels"]:
        return f"the calls differ: {[x for x in zip(got['labels'], want['labels']) if x[0] != x[1]][:1]}"
    for i, (a, b) in enumerate(zip(got["records"], want["records"])):
        if a != b:
            return f"record {i}, after {got['labels'][a[0]]}:\n  got  {a[1:]}\n  want {b[1:]}"
    return f"{len(got['records'])} records against {len(want['records'])}"


def trace():
    return json.loads(json.dumps({f"preallocate={p}": compact(run(p)) for p in (True, False)}))


if __name__ == "__main__":
    TRACE.write_text(json.dumps(trace(), separators=(",", ":")) + "\n")
    print(f"{TRACE}: {TRACE.stat().st_size} bytes")
