"""What the cases of tests/consensus_cases.py reach (no GPU), and the native host consensus at
exactly these inputs against live CPython set / Counter.  The minimums below are conditions on
the cases: when a seed misses one, the seed or the builder changes, not the condition."""
import sys

import numpy as np
import pytest

import consensus_cases as cc
from kcmc_amd import stages


def test_table_size_equals_cpython():
    """The table of a growing set, read from its allocation: 16 bytes per entry beyond the
    8-entry table that lives inside the object."""
    s, empty = set(), sys.getsizeof(set())
    for m in range(1, 6001):
        s.add(m)
        extra = sys.getsizeof(s) - empty
        assert cc.table_size(m) == (extra // 16 if extra else 8), m
    assert sorted({cc.table_size(m) for m in range(1, 6001)}) == [8, 32, 128, 512, 2048, 8192, 32768]  # never 1024
    assert [cc.table_size(m) for m in (306, 307, 1228, 1229)] == [512, 2048, 2048, 8192]
    assert [cc.scratch_words(c) for c in (8, 512, 2048, 8192)] == [0, 0, 4096, 32768]


@pytest.mark.parametrize("shape", cc.PATH_SHAPES, ids=str)
def test_path_case_reaches_its_paths(shape):
    n_tpl, nkg, F = shape
    case = cc.get_path_case(shape)
    assert case.F == F and len(case.pool) == nkg and {0, 1, 2, 3, 4, n_tpl - 1} <= case.pool
    cons, order, votes = case.consensus
    assert cons == case.pool
    # no tie at the cut: the pool wins on counts alone
    assert min(votes) > max([c for k, c in case.counter.items() if k not in case.pool], default=0)
    cl = case.classes
    assert cl.nc == nkg and cl.cap == cc.table_size(nkg)
    counts = cl.counts()
    assert all(counts[p] >= 2 for p in cc.PATHS), counts
    if F == 24:
        assert counts["frame_asc"] >= 3 and counts["cons_iter"] >= 6 and counts["frame_replay"] >= 9, counts
    # both tables grow to the consensus' table size in a frame that builds them ...
    assert cl.r_max() == cl.cap and cl.s_max() == cl.cap, (cl.r_max(), cl.s_max())
    if nkg >= 1229:
        assert cl.cap == 8192
    elif nkg in (1228, 307):
        assert cl.cap == 2048
    elif nkg == 306:
        assert cl.cap == 512
    # ... and smaller ones occur beside them
    assert len({r for p, r in zip(cl.path, cl.r_size) if p in cc.REPLAYED}) >= 3
    # cons-iter with the whole result and with a part of it
    ms = [len(case.lists[f]) for f in cl.frames("cons_iter")]
    assert max(ms) == nkg and min(ms) < nkg
    # frame-asc frames are ascending sets with a result that has a key beyond its table
    for f in cl.frames("frame_asc"):
        assert cc.is_ascending(case.sets[f]) and len(case.sets[f]) <= nkg
        assert max(case.lists[f]) >= cc.table_size(len(case.lists[f]))
    assert any(case.lists[f] != sorted(case.lists[f]) for f in cl.frames("frame_asc"))
    # the vote's queue: first frames of both kinds
    rep = set(cl.first_replayed.values())
    assert rep == {True, False}
    assert len({cl.first[k] for k, r in cl.first_replayed.items() if r}) >= 3


def test_threshold_pairs_differ_in_layout():
    words = {nkg: cc.scratch_words(cc.get_path_case((n_tpl, nkg, F)).classes.cap)
             for n_tpl, nkg, F in cc.PATH_SHAPES}
    assert (words[306], words[307], words[1228], words[1229]) == (0, 2 * 2048, 2 * 2048, 4 * 8192)


def _check_host(case, frame_base=0):
    kb, n_tpl = case.kb, case.n_tpl
    assert kb.shape == (case.F, (n_tpl + 31) // 32)
    if n_tpl % 32:
        assert not (kb[:, -1] >> np.uint32(n_tpl % 32)).any()
    v = stages.consensus_vote_host(kb, n_tpl, frame_base)
    counts = np.zeros(n_tpl, np.int64)
    for k, c in case.counter.items():
        counts[k] = c
    np.testing.assert_array_equal(v[0], counts)
    check_vote_keys(case, v, frame_base)
    cons, order, votes = case.consensus
    choice = stages.consensus_merge(v, n_tpl, case.n_kp_global, 1)
    assert choice.order.tolist() == list(order)
    assert choice.votes.tolist() == list(votes)
    assert choice.cons_iter.tolist() == list(cons)
    np.testing.assert_array_equal(choice.pack[choice.nc: choice.nc + kb.shape[1]].view(np.uint32),
                                  cc.bits([cons], n_tpl)[0])
    po, pi = stages.consensus_lookup_host(kb, n_tpl, choice.cons_iter)
    eo, ei = cc.csr(case.lists)
    np.testing.assert_array_equal(po, eo)
    np.testing.assert_array_equal(pi, ei)


def check_vote_keys(case, v, frame_base):
    """Row 1 of a vote against the classifier: key >> 32 is the first frame, and within a first
    frame the slot bits order its templates as that frame's set iterates."""
    cl = case.classes
    voted = np.zeros(case.n_tpl, bool)
    voted[list(cl.first)] = True
    assert (v[1][~voted] == np.iinfo(np.int64).max).all()
    ks = np.flatnonzero(voted)
    first = np.array([cl.first[k] for k in ks], np.int64)
    np.testing.assert_array_equal(v[1][ks] >> 32, frame_base + first)
    slot = v[1][ks] & 0xFFFFFFFF
    for f in np.unique(first):
        mine = ks[first == f]
        by_slot = mine[np.argsort(slot[first == f], kind="stable")].tolist()
        own = set(mine.tolist())
        assert by_slot == [k for k in case.sets[f] if k in own], f"first frame {f}"
        assert len(set(slot[first == f].tolist())) == len(mine)


@pytest.mark.parametrize("shape", cc.PATH_SHAPES, ids=str)
def test_host_consensus_on_path_cases(shape):
    _check_host(cc.get_path_case(shape), frame_base=0)
    _check_host(cc.get_path_case(shape), frame_base=2**31 - 1 - shape[2])


@pytest.mark.parametrize("F", cc.EDGE_F)
def test_host_consensus_on_size_edges(F):
    _check_host(cc.get_size_edge_case(F))


@pytest.mark.parametrize("n_tpl", cc.WORD_N_TPL)
def test_host_consensus_on_word_edges(n_tpl):
    case = cc.get_word_edge_case(n_tpl)
    assert sum(n_tpl - 1 in s for s in case.sets) == 2 and case.counter[n_tpl - 1] == 2
    _check_host(case)


@pytest.mark.parametrize("F", cc.EDGE_F)
def test_size_edge_case_places_its_frames(F):
    case = cc.get_size_edge_case(F)
    assert case.F == F and case.n_tpl == cc.EDGE_N_TPL
    n = [len(x) for x in case.lists]
    assert n == [len(s) for s in case.sets]  # every voted template is in the consensus
    for b in cc.edge_boundaries(F):
        assert n[b - 1] == 1 and n[b] > 1, b
        if b + 1 < F:
            assert n[b + 1] <= 1, b
    if F % 16 == 0:
        assert n[F - 1] == 1
    # the boundaries of a lane (16), a wave's pass (1024) and a vote chunk (64) are among them
    assert {b for b in (16, 64, 1024, 2048) if b < F} <= set(cc.edge_boundaries(F))
    # templates whose only frame is a chunk's last, first or second one, or the last frame
    for f, t in cc._only_at(F).items():
        assert case.counter[t] == 1 and t in case.sets[f] and case.classes.first[t] == f
    assert set(cc._only_at(F)) == {f for f in (63, 64, 65, 127, 128, F - 1) if 0 <= f < F}
    # first frames of both kinds, so both halves of vote_key_kernel run
    if F > 16:
        assert set(case.classes.first_replayed.values()) == {True, False}
