"""The stage-B pair prune of the timed build (vargeno_amd/csrc/vg_wave.h, where `pend` is formed), on the CPU.

(1) vg_quiet_chunks (vg_quiet.h) and its union over a key's exact contexts against a position-by-position scan, under sanitizers
    (tests/pair_prune_check.cpp).
(2) The two premises of the rule, against the vote itself -- `aggregate_vote` of tests/test_vote_aggregate.py, which that file pins
    to the reference's own state machine, and the oracle's replay of it:
      R2  a pass whose only key has exact contexts of two different chunks is processed at that key whatever its gate-open chunks
          find: neighbour votes can be added or removed at will;
      R1  a pass ends "no winner, or a winner among the keys the exact contexts opened" whatever the neighbours do (the retry that a
          missing winner would cause in pass 0 does not exist in pass 1);
    and, so that nobody widens the premises later, the two cases the rule leaves alone, each with a sequence in which one neighbour
    vote does change the outcome: a single key with one exact chunk, and several keys (pass 0)."""
import itertools
import os
import subprocess

import numpy as np

from conftest import CSRC
from test_vote_aggregate import aggregate_vote


def test_free_chunk_bits_equal_a_scan_for_every_key_under_sanitizers(tmp_path):
    """tests/pair_prune_check.cpp: the hand-made pile-ups of quiet_bits_check.cpp (0 .. 449 positions; empty, full, one site at every
    position, pairs, random), every key from 0 to past the end and keys left of position 0, every (chunk, n) for n = 1 .. 5: a chunk's
    bit only where its 32 positions lie inside the pile-up and hold no site, A = chunks 0 .. c and B = chunks c .. n - 1 exactly,
    nothing for n outside 2 .. 4, and vg_quiet_key == "covers all n chunks".  -fsanitize=address,undefined, run on its own."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "pair_prune_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + CSRC,
                           os.path.join(here, "pair_prune_check.cpp"), "-o", exe])
    p = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"), capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-500:], p.stderr[-2000:])
    assert int(p.stdout.split()[1]) > 1_000_000                       # (the checks were really made)


def _votes(exact, neigh):
    """exact: {key: chunks with an exact context}; neigh: [(key, chunk)] -> the pass's votes in the kernel's order: chunk by chunk,
    a chunk's exact contexts before its neighbour contexts.  (index, k-mer position, neighbour flag) arrays."""
    seq = []
    chunks = sorted({c for cs in exact.values() for c in cs} | {c for _, c in neigh})
    for c in chunks:
        seq += [(k, k + 32 * c, 0) for k, cs in exact.items() if c in cs]
        seq += [(k, k + 32 * c, 1) for k, cc in neigh if cc == c]
    a = np.array(seq, dtype=np.uint32).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2].astype(np.uint8)


def _outcome(exact, neigh):
    """(processed, winner) by per-key totals, checked against the oracle's replay of the reference's state machine."""
    from oracle import oracle as O

    idx, kpos, ng = _votes(exact, neigh)
    has, win, f, amb, most = aggregate_vote(idx, kpos, ng)
    assert most <= 255
    got = O.vote_replay(idx, kpos, ng)
    assert bool(got[0]) == has and (not has or (bool(got[3]) == amb and (amb or int(got[1]) == win))), (exact, neigh, got, (has, win, f, amb))
    processed = has and not amb
    return processed, (win if processed else None)


def _subsets(rng, items, k=6):
    """The empty set, the full set, every single item left out / alone, and k random subsets."""
    out = [[], list(items)] + [[x for j, x in enumerate(items) if j != i] for i in range(len(items))] + [[x] for x in items]
    for _ in range(k):
        out.append([x for x in items if rng.random() < 0.5])
    return out


def test_r2_one_key_with_two_exact_chunks_is_processed_whatever_the_neighbours_vote():
    rng = np.random.default_rng(41)
    checked = 0
    for trial in range(200):
        n = int(rng.integers(2, 5))
        key = int(rng.integers(100_000, 200_000))
        chunks = sorted(rng.choice(n, size=int(rng.integers(2, n + 1)), replace=False).tolist())
        # neighbour contexts as stage B keeps them (implied position = the key) and as it drops them (another position): any chunk, repeated
        stray = key + int(rng.integers(1, 500))
        pool = [(key if rng.random() < 0.7 else stray, int(rng.integers(0, n))) for _ in range(int(rng.integers(1, 7)))]
        for sub in _subsets(rng, pool):
            assert _outcome({key: chunks}, sub) == (True, key), (key, chunks, sub)
            checked += 1
    assert checked > 2000


def test_r1_every_outcome_is_no_winner_or_a_winner_among_the_exact_keys():
    rng = np.random.default_rng(42)
    winners = none = 0
    for trial in range(200):
        n = int(rng.integers(2, 5))
        keys = (rng.choice(4000, size=int(rng.integers(1, 5)), replace=False) + 100_000).tolist()
        exact = {int(k): sorted(rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False).tolist()) for k in keys}
        strays = [int(k) + 7 for k in keys]
        pool = [(int(rng.choice(keys + strays)), int(rng.integers(0, n))) for _ in range(int(rng.integers(1, 8)))]
        for sub in _subsets(rng, pool):
            processed, win = _outcome(exact, sub)
            assert (not processed and win is None) or win in exact, (exact, sub, win)
            winners += processed
            none += not processed
    assert winners > 500 and none > 500


def test_the_two_cases_the_rule_leaves_alone_do_depend_on_a_neighbour():
    key, other = 150_000, 150_321
    # one key, one exact chunk: not live on its own; a neighbour context of a LATER chunk makes it live, an earlier one is refused
    assert _outcome({key: [1]}, []) == (False, None)
    assert _outcome({key: [1]}, [(key, 2)]) == (True, key)
    assert _outcome({key: [1]}, [(key, 0)]) == (False, None)
    # several keys (pass 0): a neighbour breaks the tie of two live keys, makes a tie, or changes the winner -- and with the tie, the retry
    two = {key: [0, 1], other: [0, 1]}
    assert _outcome(two, []) == (False, None)
    assert _outcome(two, [(other, 1)]) == (True, other)
    assert _outcome({key: [0, 1, 2], other: [0, 1]}, []) == (True, key)
    assert _outcome({key: [0, 1, 2], other: [0, 1]}, [(other, 2)]) == (False, None)
    assert _outcome({key: [0, 1, 2], other: [0, 1]}, [(other, 2), (other, 3)]) == (True, other)
    # exhaustively over small cases: both excluded premises have neighbour sets that flip "processed" or the winner
    flips = {"one_chunk": 0, "several_keys": 0}
    for n in (2, 3, 4):
        for c in range(n):
            base = _outcome({key: [c]}, [])
            flips["one_chunk"] += any(_outcome({key: [c]}, [(key, j)]) != base for j in range(n))
        for ca, cb in itertools.product(itertools.combinations(range(n), 2), repeat=2):
            ex = {key: list(ca), other: list(cb)}
            base = _outcome(ex, [])
            flips["several_keys"] += any(_outcome(ex, [(k, j)]) != base for k in (key, other) for j in range(n))
    assert flips["one_chunk"] >= 6 and flips["several_keys"] >= 10, flips
