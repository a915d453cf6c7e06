"""CPU: hop_eval_place -- the stream an evaluation group of hop_encode_frame is issued on: the one whose uncollected chains are expected to end first, by the table of
expected lengths per class in host/hop_hostlogic.cpp -- against a restatement in numpy, over the group sequences the rounds of a CTU's quadtree nodes produce."""
import itertools
import os
import sys

import numpy as np
import pytest

from hoputil import ROOT

sys.path.insert(0, os.path.join(ROOT, "hevc-hop_amd"))
import hophip as hp  # noqa: E402

INTER, INTRA = hp.HOP_EVAL_INTER, hp.HOP_EVAL_INTRA
# the table restated: ms per chain by CU size 8, 16, 32, 64; rows: SS/GT with residual, without, intra 2Nx2N, intra NxN
TABLE = np.array([[0.325, 1.779, 5.540, 14.346],
                  [0.05, 0.05, 0.06, 0.08],
                  [0.522, 1.794, 5.502, 17.433],
                  [0.722, 0.722, 0.722, 0.722]])
PITCH = 16


def expected_ms(cls):
    kind, log2_cu, flag, n = cls
    fills = -(-n // 1024) if n > 1024 else 1                              # candidates side by side: a group is as long as its longest walk until the device is full
    return TABLE[(2 if kind == INTRA else 0) + (1 if flag else 0), min(max(log2_cu, 3), 6) - 3] * fills


def place(cls, busy_classes):
    """the restatement: busy_classes[s] = classes issued on stream s and not collected; smallest sum of expected lengths, ties to the lowest index"""
    busy = np.array([sum(expected_ms(c) for c in q) for q in busy_classes])
    return int(np.argmin(busy)), busy                                       # (argmin returns the first of equals)


def lib():
    return hp.load()


def lib_place(L, cls, busy_classes):
    return hp.eval_place(L, cls, busy_classes, PITCH)                       # (fills what lies beyond a stream's classes with values that are no class: it must not be read)


def node_sequences(log2_cu):
    """the groups of the rounds of a node of this size with its speculated first sub-CU, in arrival order: the intra groups early (any order), then the SS/GT groups with
    and without residual of both sizes in the round that ends the node.  A stand-alone 8x8 node has no child."""
    n_inter, n_intra = 48, 16
    sizes = [log2_cu, log2_cu - 1] if log2_cu > 3 else [3]
    early = [(INTRA, s, 0, n_intra) for s in sizes] + ([(INTRA, 3, 1, n_intra)] if 3 in sizes else [])
    late = [(INTER, s, f, n_inter) for s in sizes for f in (0, 1)]
    return [list(p) + late for p in itertools.permutations(early)]


def run_sequence(L, seq, S):
    """places a sequence from empty streams through the library, checking every step against the restatement; returns the per-stream classes"""
    streams = [[] for _ in range(S)]
    for cls in seq:
        want, busy = place(cls, streams)
        got = lib_place(L, cls, streams)
        assert got == want, (cls, streams)
        assert busy[got] <= busy.min()                                      # no group goes to a stream busier than another at that moment
        streams[got].append(cls)
    return streams


def makespan(streams):
    return max(sum(expected_ms(c) for c in q) for q in streams)


def test_the_table_is_the_restated_one():
    L = lib()
    for kind in (INTER, INTRA):
        for log2_cu in (3, 4, 5, 6):
            for flag in (0, 1):
                for n in (1, 48, 1024, 1025, 2048):
                    assert hp.eval_expected_ms(L, (kind, log2_cu, flag, n)) == pytest.approx(expected_ms((kind, log2_cu, flag, n)), rel=1e-12)
    assert expected_ms((INTER, 6, 0, 2048)) == 2 * expected_ms((INTER, 6, 0, 1024))


@pytest.mark.parametrize("log2_cu,n_groups", [(6, 6), (5, 6), (4, 7), (3, 4)])
def test_node_rounds_are_placed_greedily_and_no_worse_than_round_robin(log2_cu, n_groups):
    L = lib()
    seqs = node_sequences(log2_cu)
    assert len(seqs) == {6: 2, 5: 2, 4: 6, 3: 2}[log2_cu] and all(len(s) == n_groups for s in seqs)
    for seq in seqs:
        for S in (2, 4, 8):
            streams = run_sequence(L, seq, S)
            assert sorted(c for q in streams for c in q) == sorted(seq)
            if S != 4: continue                                             # (the default; on two streams a greedy placement can lose to a lucky deal -- list scheduling is within 4/3 - 1/3S of the optimum, not at it)
            # the two longest classes of the round never share a stream
            a, b = sorted(seq, key=expected_ms)[-2:]
            assert [a in q for q in streams] != [b in q for q in streams]
            # the predicted makespan is no larger than under round-robin dealing from any starting offset
            for off in range(4):
                rr = [[] for _ in range(S)]
                for i, cls in enumerate(seq): rr[(off + i) % S].append(cls)
                assert makespan(streams) <= makespan(rr) + 1e-12, (seq, S, off)
        # with four streams the long chains end up alone: the round is as long as its longest chain
        assert makespan(run_sequence(L, seq, 4)) == max(expected_ms(c) for c in seq)


def test_ties_go_to_the_lowest_index_and_streams_in_use_are_counted():
    L = lib()
    assert lib_place(L, (INTER, 4, 0, 8), [[], [], [], []]) == 0
    assert lib_place(L, (INTER, 4, 0, 8), [[(INTRA, 6, 0, 4)], [], [], []]) == 1
    same = (INTER, 5, 0, 8)
    assert lib_place(L, (INTRA, 3, 0, 8), [[same], [same], [same], [same]]) == 0
    # two short chains against one long one; a stream left from an earlier round counts like any other
    assert lib_place(L, (INTER, 3, 0, 8), [[(INTRA, 6, 0, 4)], [(INTER, 4, 0, 8), (INTER, 4, 1, 8)], [(INTRA, 5, 0, 4)], [(INTER, 5, 0, 8)]]) == 1
    # random states against the restatement
    rng = np.random.default_rng(11)
    for _ in range(300):
        S = int(rng.integers(1, 9))
        streams = [[(int(rng.integers(0, 2)), int(rng.integers(3, 7)), int(rng.integers(0, 2)), int(rng.integers(1, 2049))) for _ in range(int(rng.integers(0, 5)))] for _ in range(S)]
        cls = (int(rng.integers(0, 2)), int(rng.integers(3, 7)), int(rng.integers(0, 2)), int(rng.integers(1, 2049)))
        assert lib_place(L, cls, streams) == place(cls, streams)[0]
