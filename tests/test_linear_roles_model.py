"""CPU model of csrc/linear_roles.h: the C-slot maps of the MFMA and store wavefronts (every element read out is the one
written there, bank-conflict-free in the service groups of ds_write_b128 / ds_read_b128) and the FULL / FREE handshake
(replayed under random interleavings: no slot is overwritten before it is read out, every tile is stored once, nothing
waits forever)."""
import random

NW, NS, BM = 8, 4, 64
SLOT = BM * 32 * 4


def _write_addr(wave, i, g, lane):
    """MFMA wavefront: lane's 16-byte piece (tile i, register group g) -> (slot byte address, row, 16-byte chunk)."""
    r = i * 32 + (lane & 31)
    c = 2 * g + (lane >> 5)
    return wave * SLOT + r * 128 + ((c ^ (r & 7)) << 4), r, c


def _read_addr(wave, p, lane):
    """Store wavefront: pass p, lane -> (slot byte address, row, chunk)."""
    rr, c = lane >> 3, lane & 7
    r = p * 8 + rr
    return wave * SLOT + rr * 128 + ((c ^ rr) << 4) + p * 1024, r, c


def test_slot_maps_round_trip():
    written = {}
    for i in range(2):
        for g in range(4):
            for lane in range(64):
                a, r, c = _write_addr(3, i, g, lane)
                assert a not in written and 3 * SLOT <= a < 4 * SLOT
                written[a] = (r, c)
    assert len(written) == BM * 8
    seen = set()
    for p in range(8):
        for lane in range(64):
            a, r, c = _read_addr(3, p, lane)
            assert written[a] == (r, c)
            seen.add(a)
    assert seen == set(written)


def test_slot_accesses_are_bank_conflict_free():
    # ds_write_b128: groups of 8 consecutive lanes, bank = (a / 4) mod 32
    for i in range(2):
        for g in range(4):
            for grp in range(8):
                banks = [(_write_addr(0, i, g, l)[0] // 4 + d) % 32 for l in range(8 * grp, 8 * grp + 8) for d in range(4)]
                assert len(set(banks)) == 32
    # ds_read_b128: four groups of 16 lanes, bank = (a / 4) mod 64
    groups = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
              list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
    groups += [[l + 32 for l in gr] for gr in groups]
    for p in range(8):
        for gr in groups:
            banks = [(_read_addr(0, p, l)[0] // 4 + d) % 64 for l in gr for d in range(4)]
            assert len(set(banks)) == 64


def _run_protocol(nct, seed):
    rnd = random.Random(seed)
    full, free = [0] * NW, [0] * NW
    slot = [None] * NW                           # tile index held in the slot
    stored = []
    # MFMA wavefront state: next tile t, phase 'compute' -> 'wait_free' -> publish
    mt = [0] * NW
    ntiles = [(nct - w + NW - 1) // NW if w < nct else 0 for w in range(NW)]
    done_m = [ntiles[w] == 0 for w in range(NW)]
    d = [[0, 0] for _ in range(NS)]
    done_s = [all(ntiles[w] == 0 for w in (s, s + 4)) for s in range(NS)]
    for _ in range(100000):
        if all(done_m) and all(done_s):
            break
        actors = [("m", w) for w in range(NW) if not done_m[w]] + [("s", s) for s in range(NS) if not done_s[s]]
        kind, k = rnd.choice(actors)
        if kind == "m":
            t = mt[k]
            if free[k] < t:                      # FREE: the slot still holds an unread tile -> sleep
                continue
            assert slot[k] is None
            slot[k] = t
            full[k] = t + 1
            mt[k] += 1
            done_m[k] = mt[k] == ntiles[k]
        else:
            for j, w in enumerate((k, k + 4)):
                if d[k][j] < ntiles[w] and full[w] > d[k][j]:
                    assert slot[w] == d[k][j]
                    stored.append(w + NW * slot[w])
                    slot[w] = None
                    d[k][j] += 1
                    free[w] = d[k][j]
            done_s[k] = all(d[k][j] == ntiles[w] for j, w in enumerate((k, k + 4)))
    else:
        raise AssertionError("handshake did not finish")
    assert sorted(stored) == list(range(nct))


def test_handshake_under_random_interleavings():
    for nct in (48, 8, 3, 1):
        for seed in range(20):
            _run_protocol(nct, seed)
