"""A restatement of the LDS traffic of prefill_attn_pipe_kernel (csrc/prefill.hip, behind "prologue: K halves 0, 1, 2 and V tile
0"), in the manner of tests/test_decode_schedule_host.py: which 32-key K half each quarter of the K region holds, which V tile
each V buffer holds, which wave requests them and which reads them.  The kernel's loop and the table below change together.

A workgroup with nt key tiles has 2 nt halves.  K half h lives in quarter h & 3, V tile t in buffer t & 1.  Every wave, live or
not, issues its piece of every request and joins every barrier; only a live wave reads, and under a causal mask only up to
the half its last row reaches.  The rule the kernel's comment at PF_DMA states, checked here for nt = 0 .. 9 and every pattern of
live and idle waves that prefill_rows can produce:
  * a read finds the half it expects, and the request that brought it is separated from the read by that wave's wait and a barrier;
  * no request into a region shares a barrier epoch with another wave's read of what the region held before.
The schedule is written down twice: as the kernel stood before the prologue barrier (one hazard: K half 4 into quarter 0 against
the prologue's read of half 0, from three tiles on - profiles/prefill_prologue_race.txt) and as it stands."""
import pytest

WAVES = 8
# what a wave does, in program order; K entries are halves, V entries tiles, both relative to iteration t (K: + 2 t, V: + t)
FIXED = dict(
    prologue_dma=(("K", 0), ("K", 1), ("K", 2), ("V", 0)),      # then wait, barrier
    prologue_read=("K", 0),                                     # scores of half 0
    prologue_barrier=True,
    burst=(("K", 3), ("K", 4), ("V", 1)),                       # PF_DMA(t)
    steps=((("K", 1), ("V", 0)), (("K", 2), ("V", 0))),         # half-steps 2 t, 2 t + 1: scores of the next half, values of this one
)                                                               # then wait, barrier (PF_SYNC)
PARENT = dict(FIXED, prologue_barrier=False)


def region(side, n):
    return f"K{n & 3}" if side == "K" else f"V{n & 1}"


def wave_events(sched, nt, reach):
    """reach: the number of halves the wave's rows attend to (0: an idle wave).  -> [(kind, region, side, n)] with kind in
    dma / read / wait / barrier; a request past the workgroup's last half or tile is not issued (dma_k_half, dma_v_tile)."""
    ev = []
    exists = lambda side, n: n < (2 * nt if side == "K" else nt)
    dma = lambda side, n: ev.append(("dma", region(side, n), side, n)) if exists(side, n) else None
    # half-step h reads the K half h + 1 and the V rows of half h while half h is live; a K half past the wave's reach is read
    # too, but masked whole: what it holds does not matter, so it is no event
    read = lambda side, n, h: ev.append(("read", region(side, n), side, n)) if h < reach and (side == "V" or n < reach) else None
    for side, n in sched["prologue_dma"]:
        dma(side, n)
    ev += [("wait",), ("barrier",)]
    read(*sched["prologue_read"], 0)
    if sched["prologue_barrier"]:
        ev.append(("barrier",))
    for t in range(nt):
        for side, n in sched["burst"]:
            dma(side, n + (2 * t if side == "K" else t))
        for j, step in enumerate(sched["steps"]):
            for side, n in step:
                read(side, n + (2 * t if side == "K" else t), 2 * t + j)
        ev += [("wait",), ("barrier",)]
    return ev


def hazards(sched, nt, reaches):
    """-> the set of (what, region, side, half or tile requested, half or tile the read expects)."""
    dmas, reads = [], []      # (wave, program index, epoch, region, side, n[, epoch from which the bytes may be read])
    for w, reach in enumerate(reaches):
        epoch, pending = 0, []
        for i, e in enumerate(wave_events(sched, nt, reach)):
            if e[0] == "dma":
                pending.append([w, i, epoch, e[1], e[2], e[3], None])
            elif e[0] == "wait":
                for d in pending:
                    d[6] = epoch + 1      # landed for this wave; everyone else knows it behind the next barrier
                dmas += pending
                pending = []
            elif e[0] == "barrier":
                epoch += 1
            else:
                reads.append((w, i, epoch, e[1], e[2], e[3]))
        assert not pending, "a request nobody waits for"
    assert len({sum(e[0] == "barrier" for e in wave_events(sched, nt, r)) for r in reaches}) == 1, "waves disagree about the barriers"
    found = set()
    for w, i, epoch, reg, side, n in reads:
        for u in range(len(reaches)):      # every wave brings its own piece of the region
            # u's requests into the region that may have been issued when the read runs: earlier epochs, and the same epoch
            # unless it is the reader's own, later in its program
            mine = [d for d in dmas if d[0] == u and d[3] == reg and (d[2] < epoch or (d[2] == epoch and (u != w or d[1] < i)))]
            if not mine:
                found.add(("never requested", reg, side, None, n))
                continue
            last = mine[-1]
            if (last[4], last[5]) != (side, n):
                found.add(("overwritten" if last[2] == epoch else "stale", reg, side, last[5], n))
            elif last[6] > epoch:
                found.add(("not waited for", reg, side, last[5], n))
    return found


def live_patterns(nt):
    """The reaches of the 8 waves for hpw = 8, 4, 2, 1 heads per workgroup (8 / hpw waves per head) with 1 .. 8 / hpw of a head's
    waves holding rows (wave_live = q_lo < n_q), without a mask (every live wave reads every half) and under a causal one (the
    last live wave of a head reaches the last half or the one before it, each wave before it 32 keys less)."""
    nh2 = 2 * nt
    for hpw in (8, 4, 2, 1):
        wph = WAVES // hpw
        for k in range(1, wph + 1):
            yield [nh2 if w % wph < k else 0 for w in range(WAVES)]
            for short in (0, 1):
                yield [max(min(nh2, 1), nh2 - short - (k - 1 - w % wph)) if w % wph < k else 0 for w in range(WAVES)]


@pytest.mark.parametrize("nt", range(10))
def test_fixed_schedule_has_no_hazard(nt):
    for reaches in live_patterns(nt):
        assert hazards(FIXED, nt, reaches) == set(), (nt, reaches)


@pytest.mark.parametrize("nt", range(10))
def test_parent_schedule_has_the_one_hazard_from_three_tiles_on(nt):
    """Without the prologue barrier the first burst's K half 4 lands in quarter 0 in the epoch of the prologue's read of half 0."""
    want = {("overwritten", "K0", "K", 4, 0)} if nt >= 3 else set()
    for reaches in live_patterns(nt):
        assert hazards(PARENT, nt, reaches) == want, (nt, reaches)


def test_every_half_and_tile_is_read_by_a_full_wave():
    """The model reads what the kernel multiplies: halves 0 .. 2 nt - 1 and, per half, its tile's V buffer."""
    for nt in range(1, 10):
        ev = [e for e in wave_events(FIXED, nt, 2 * nt) if e[0] == "read"]
        assert [e[3] for e in ev if e[2] == "K"] == list(range(2 * nt))
        assert [e[3] for e in ev if e[2] == "V"] == [t for t in range(nt) for _ in range(2)]


def test_checker_catches_a_longer_prefetch_and_a_missing_request():
    """Controls: a burst one half further ahead writes a quarter that this iteration still reads; a prologue that leaves a half
    out lets its reader find nothing."""
    ahead = dict(FIXED, burst=(("K", 4), ("K", 5), ("V", 1)), prologue_dma=FIXED["prologue_dma"] + (("K", 3),))
    assert ("overwritten", "K1", "K", 5, 1) in hazards(ahead, 4, [8] * WAVES)
    ev = wave_events(FIXED, 2, 4)
    assert ev.count(("wait",)) == 3 and ev.count(("barrier",)) == 4
    late = dict(FIXED, prologue_dma=FIXED["prologue_dma"][1:])      # half 0 is never brought
    assert hazards(late, 1, [2] * WAVES) == {("never requested", "K0", "K", None, 0)}
