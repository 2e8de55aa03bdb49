"""A restatement of the lean decode kernel's block loop (csrc/attn_lean.h, behind "A wave with n units runs") as a model of the
two ring slots, in the style of the protocol models of tests/test_host_logic.py: which unit's K and V bytes a slot holds, who
requested them and who reads them.  The kernel's loop and this one change together.

A wave with n units runs: the prologue (request unit 0 into slot 0, scores of unit 0, request round 1 into slot 1 - clamped to
the wave's last unit by LAUNCH_FRONT_ROUND when n < 2), n - 1 blocks (block k: values of unit k in slot k & 1 beside the scores
of unit k + 1 in the other slot; a requesting block asks for unit k + 2 into slot k & 1: K at its start, V once the last value
gather of unit k is out), the values of unit n - 1 alone.  Blocks 0 .. n - 3 request, block n - 2 is a BLOCK_LAST, which requests
nothing.  For n = 0 .. 66 (a wave has at most 64 rounds):
  * every unit j < n is requested exactly once, into slot j & 1, before the step that consumes it;
  * no block requests a unit >= n (nor any unit a second time);
  * the slot of the closing value pass holds unit n - 1."""
import pytest

RING = 2


class _Wave:
    def __init__(self, n):
        self.n = n
        self.K, self.V = [None, None], [None, None]      # unit whose bytes the slot's registers hold
        self.requests = []                               # (side, round asked for, unit that came, slot, who)
        self.reads = []                                  # (side, unit, slot, what)
        self.bl_j = 0
        self.tail_requested_at = None                    # blocks run when tail_request was issued

    # LAUNCH_FRONT_ROUND: round J of this wave, or its last one
    def _round(self, j):
        return j if j < self.n else max(self.n - 1, 0)

    def req_k(self, slot, j, who):
        self.K[slot] = self._round(j)
        self.requests.append(("K", j, self._round(j), slot, who))

    def req_v(self, slot, j, who):
        self.V[slot] = self._round(j)
        self.requests.append(("V", j, self._round(j), slot, who))

    def read(self, side, slot, unit, what):
        held = (self.K if side == "K" else self.V)[slot]
        self.reads.append((side, unit, slot, what))
        assert held == unit, f"n={self.n}: {what} reads {side} of unit {unit} from slot {slot}, which holds unit {held}"

    def block(self, sl, last):
        j, sln = self.bl_j, 1 - sl
        if not last:
            self.req_k(sl, j + RING, "block")            # UNIT_REQ_K(BL_SL, bl_j + RING): unit j's K bytes were used up by the block before
        self.read("V", sl, j, "value gathers")           # VG(BL_SL, 2 ..): unit j (gathers 0, 1 were issued by the step before)
        if not last:
            self.req_v(sl, j + RING, "block")            # step NV - 3: the last value gather of unit j is out
        self.read("K", sln, j + 1, "score gathers")      # KG(BL_SLN, 3 ..): unit j + 1
        if not last:
            self.read("K", sl, j + 2, "closing score gathers")      # KG(BL_SL, 0 .. 2) of round j + 2
        self.read("V", sln, j + 1, "closing value gathers")         # VG(BL_SLN, 0), VG(BL_SLN, 1)
        self.bl_j += 1

    def run(self):
        n = self.n
        nb = n - 1 if n > 1 else 0
        self.req_k(0, 0, "prologue")
        self.req_v(0, 0, "prologue")
        if n > 0:
            self.read("K", 0, 0, "prologue scores")
        self.req_k(1, 1, "prologue")                     # SA_STEP 4 / 12
        self.req_v(1, 1, "prologue")
        va = None
        if n > 0:
            self.read("V", 0, 0, "VG(0, 0), VG(0, 1)")
            if nb > 0:
                self.read("K", 1, 1, "KG(1, 0 .. 2)")
                rq = nb - 1
                while rq > 0:
                    self.block(0, last=False)
                    if rq == 1:
                        break
                    self.block(1, last=False)
                    rq -= 2
                if not n & 1:
                    self.block(0, last=True)
            self.tail_requested_at = self.bl_j
            if n & 1:
                if nb > 0:
                    self.block(1, last=True)
                va = 0
            else:
                va = 1
            self.read("V", va, n - 1, "closing value pass")
        return va


@pytest.mark.parametrize("n", range(67))
def test_every_unit_requested_once_and_read_from_its_slot(n):
    w = _Wave(n)
    va = w.run()      # (every read asserts that its slot holds the unit it wants)
    nb = max(n - 1, 0)
    assert w.bl_j == nb
    if n > 0:
        assert va == (n - 1) & 1
    for side in ("K", "V"):
        got = [(unit, slot) for s_, j, unit, slot, who in w.requests if s_ == side and j < n]
        assert got == [(j, j & 1) for j in range(n)], (n, side, got)      # once each, in order, unit j into slot j & 1
    # a block never asks for a round the wave does not have; only the prologue's round 1 is clamped (waves with 0 or 1 units)
    assert all(j < n for _s, j, _u, _sl, who in w.requests if who == "block")
    clamped = [(s_, j, who) for s_, j, _u, _sl, who in w.requests if j >= n]
    assert clamped == ([("K", 0, "prologue"), ("V", 0, "prologue")] if n == 0 else []) + (
        [("K", 1, "prologue"), ("V", 1, "prologue")] if n < 2 else [])
    # requesting blocks: n - 2 of them (units 2 .. n - 1), one K and one V request each
    assert sum(1 for r in w.requests if r[4] == "block") == 2 * max(n - 2, 0)
    # every unit's scores and values were read
    for j in range(n):
        assert ("K", j, j & 1) in {r[:3] for r in w.reads} and ("V", j, j & 1) in {r[:3] for r in w.reads}
    # tail_request sits where it sat: in front of the last block of an odd wave, behind the last block of an even one
    if n > 0:
        assert w.tail_requested_at == (nb - 1 if (n & 1 and nb) else nb)


def test_model_catches_a_missing_request():
    """The negative control: a loop whose last REQUESTING block is a BLOCK_LAST too reads a stale slot."""
    w = _Wave(4)
    w.req_k(0, 0, "prologue"), w.req_v(0, 0, "prologue"), w.req_k(1, 1, "prologue"), w.req_v(1, 1, "prologue")
    w.block(0, last=False)
    w.block(1, last=True)      # should have requested unit 3
    with pytest.raises(AssertionError, match="holds unit 1"):
        w.block(0, last=True)
