"""The device consensus (csrc/consensus.hip) against live CPython set / Counter, at the inputs of
tests/consensus_cases.py: every way lookup_order_kernel writes a frame's list, with the set
tables in LDS, half in scratch and both in scratch (and on both sides of the two thresholds),
the frame, chunk, pass, block and word edges of the scan and vote kernels, the largest frame
base and the largest vote the launcher admits, and sharded votes.
tests/test_consensus_cases_host.py holds what the cases reach."""
import numpy as np
import pytest
import torch

import consensus_cases as cc
from kcmc_amd import _lib, stages
from test_consensus_cases_host import check_vote_keys

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1
INT64_MAX = np.iinfo(np.int64).max


def _dev_bits(kb, dev):
    return torch.from_numpy(kb.view(np.int32).copy()).to(dev)  # the case's bitmask is read-only


def _host_choice(case, v=None):
    if v is None:
        v = stages.consensus_vote_host(case.kb, case.n_tpl)
    return stages.consensus_merge(v, case.n_tpl, case.n_kp_global, 1)


def _check_lookup(case, dev, choice=None):
    choice = choice or _host_choice(case)
    assert choice.cons_iter.tolist() == list(case.consensus[0])
    kb, pack = _dev_bits(case.kb, dev), torch.from_numpy(choice.pack).to(dev)
    po_t, pi_t = stages.consensus_lookup(kb, case.n_tpl, pack, choice.nc)
    po, pi = po_t.cpu().numpy(), pi_t.cpu().numpy()
    eo, ei = cc.csr(case.lists)
    np.testing.assert_array_equal(po, eo)
    cl = case.classes
    bad = {}
    for f, want in enumerate(case.lists):
        if pi[eo[f]:eo[f + 1]].tolist() != want:
            bad.setdefault(cl.path[f], []).append(f)
    assert not bad, "; ".join(f"{len(fs)} frames of path {p} differ, first {fs[0]}" for p, fs in bad.items())
    np.testing.assert_array_equal(pi[: eo[-1]], ei)
    po2, pi2 = stages.consensus_lookup(kb, case.n_tpl, pack, choice.nc)
    assert torch.equal(po2, po_t) and torch.equal(pi2[: eo[-1]], pi_t[: eo[-1]])
    return po, pi[: eo[-1]]


def _check_vote(case, dev, frame_base=0):
    got = stages.consensus_vote(_dev_bits(case.kb, dev), case.n_tpl, frame_base).cpu().numpy()
    counts = np.zeros(case.n_tpl, np.int64)
    for k, c in case.counter.items():
        counts[k] = c
    np.testing.assert_array_equal(got[0], counts)
    check_vote_keys(case, got, frame_base)
    np.testing.assert_array_equal(got, stages.consensus_vote_host(case.kb, case.n_tpl, frame_base))
    return got


# ------------------------------------------------------------------ lookup paths
@pytest.mark.parametrize("shape", cc.PATH_SHAPES, ids=str)
def test_lookup_paths_equal_cpython(dev, shape):
    case = cc.get_path_case(shape)
    _check_lookup(case, dev)
    F, nc, cap = case.F, case.classes.nc, case.classes.cap
    words = 0 if nc <= 306 else 2 * cap if nc <= 1228 else 4 * cap
    assert cap == cc.table_size(nc) and words == cc.scratch_words(cap)
    assert _lib.load().kcmc_consensus_lookup_scratch_bytes(F, nc) == 4 * F * words


@pytest.mark.parametrize("shape", cc.PATH_SHAPES, ids=str)
def test_vote_paths_equal_cpython(dev, shape):
    _check_vote(cc.get_path_case(shape), dev, frame_base=0)
    _check_vote(cc.get_path_case(shape), dev, frame_base=977)


# ------------------------------------------------------------------ size edges
@pytest.mark.parametrize("F", cc.EDGE_F)
def test_frame_count_edges(dev, F):
    case = cc.get_size_edge_case(F)
    _check_lookup(case, dev, _host_choice(case, _check_vote(case, dev, frame_base=3)))


@pytest.mark.parametrize("n_tpl", cc.WORD_N_TPL)
def test_template_count_edges(dev, n_tpl):
    case = cc.get_word_edge_case(n_tpl)
    _check_lookup(case, dev, _host_choice(case, _check_vote(case, dev)))


# ------------------------------------------------------------------ frame_base
def test_vote_largest_frame_base(dev):
    case = cc.get_path_case(cc.PATH_SHAPES[0])
    F, n_tpl = case.F, case.n_tpl
    got = _check_vote(case, dev, frame_base=INT32_MAX - F)
    assert (got[1] >= 0).all() and (got[1][got[0] > 0] < INT64_MAX).all()
    assert (got[1][got[0] > 0] >> 32).max() == INT32_MAX - F + max(case.classes.first.values())
    # one more: refused by the launcher's size check, before anything is written.  The C entry
    # answers KCMC_EINVAL, which kcmc_amd._lib.check raises as ValueError
    kb = _dev_bits(case.kb, dev)
    out = torch.full((2, n_tpl), -7, dtype=torch.int64, device=dev)
    rc = _lib.load().kcmc_consensus_vote(stages._ctx(dev).handle, stages._ptr(kb), F, n_tpl, INT32_MAX - F + 1,
                                         stages._ptr(out), stages._stream(dev))
    assert rc == _lib.KCMC_EINVAL and b"bad sizes" in _lib.load().kcmc_last_error()
    with pytest.raises(ValueError, match="bad sizes"):
        stages.consensus_vote(kb, n_tpl, INT32_MAX - F + 1, out=out)
    torch.cuda.synchronize(dev)
    assert (out == -7).all()


# ------------------------------------------------------------------ the largest vote
def _vote_lds_bytes(F, n_tpl):
    return 8 * n_tpl + 4 * ((F + 31) // 32) + 4 * min(F, n_tpl)


def test_vote_largest_launch(dev):
    """The most templates kcmc_consensus_vote admits (150 KiB of dynamic LDS for vote_key_kernel)
    at F = 32, every first frame replayed."""
    F = 32
    n_tpl = max(n for n in range(19000, 19400) if _vote_lds_bytes(F, n) <= 150 * 1024)
    assert n_tpl == 19183 and _vote_lds_bytes(F, n_tpl + 1) > 150 * 1024
    rng = np.random.default_rng(11)
    sets = [cc.as_set(rng.choice(n_tpl, 40, replace=False)) for _ in range(F)]
    sets[F - 1] = cc.as_set(sets[F - 1] | {n_tpl - 1, 0})
    case = cc.Case("largest-vote", n_tpl, 100, sets)
    assert all(case.classes.first_replayed.values())
    assert len(set(case.classes.first.values())) == F
    _check_vote(case, dev, frame_base=5)
    wide = _dev_bits(cc.bits(sets, n_tpl + 1), dev)
    with pytest.raises(_lib.KcmcError, match="too many") as e:
        stages.consensus_vote(wide, n_tpl + 1, 5)
    assert e.value.code == _lib.KCMC_EUNSUPPORTED


# ------------------------------------------------------------------ sharded votes
def test_sharded_device_votes_merge_to_the_unsharded_choice(dev):
    case = cc.get_path_case(cc.PATH_SHAPES[2])
    F, n_tpl = case.F, case.n_tpl
    cuts = [0, 13, 31, F]
    assert all(c % 64 for c in cuts[1:]) and F < 64
    kb = _dev_bits(case.kb, dev)
    votes = np.stack([stages.consensus_vote(kb[a:b].contiguous(), n_tpl, a).cpu().numpy()
                      for a, b in zip(cuts, cuts[1:])])
    choice = stages.consensus_merge(votes, n_tpl, case.n_kp_global, 1)
    whole = _host_choice(case)
    cons, order, counts = case.consensus
    assert choice.order.tolist() == whole.order.tolist() == list(order)
    assert choice.votes.tolist() == whole.votes.tolist() == list(counts)
    np.testing.assert_array_equal(choice.pack, whole.pack)
    assert choice.cons_iter.tolist() == list(cons)
    po_full, pi_full = _check_lookup(case, dev, choice)
    pack = torch.from_numpy(choice.pack).to(dev)
    parts = []
    for a, b in zip(cuts, cuts[1:]):
        po, pi = stages.consensus_lookup(kb[a:b].contiguous(), n_tpl, pack, choice.nc)
        po, pi = po.cpu().numpy(), pi.cpu().numpy()
        np.testing.assert_array_equal(po, po_full[a:b + 1] - po_full[a])
        parts.append(pi[: po[-1]])
    np.testing.assert_array_equal(np.concatenate(parts), pi_full)


def test_sharded_device_votes_across_vote_chunks(dev):
    """Ranges cut inside vote_count_kernel's 64-frame chunks of a 1025-frame case."""
    case = cc.get_size_edge_case(1025)
    cuts = [0, 65, 127, 1000, 1025]
    kb = _dev_bits(case.kb, dev)
    votes = np.stack([stages.consensus_vote(kb[a:b].contiguous(), case.n_tpl, a).cpu().numpy()
                      for a, b in zip(cuts, cuts[1:])])
    choice = stages.consensus_merge(votes, case.n_tpl, case.n_kp_global, 1)
    cons, order, counts = case.consensus
    assert choice.order.tolist() == list(order) and choice.votes.tolist() == list(counts)
    assert choice.cons_iter.tolist() == list(cons)
    np.testing.assert_array_equal(choice.pack, _host_choice(case).pack)
