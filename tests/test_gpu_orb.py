"""The ORB-style detector kernels (f1, csrc/orb.hip) against the CPU oracle at the edge
cases of tests/test_orb_host.py (which proves on the host that each case reaches the
branch it is named for), across the launcher's batch loop, on a misaligned stack, with
an empty budget, and the argument errors.  Counts, keypoints and descriptors bit-equal."""
import numpy as np
import pytest
import torch

import test_orb_host as host
from kcmc_amd import _lib, orb, stages

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _assert_frame_matches_oracle(k, f, img, p, tag):
    cnt = int(k.count[f].cpu())
    rkp, rdes = host.detect_oracle(img, p)
    assert cnt == len(rkp), (tag, f, cnt, len(rkp))
    assert np.array_equal(k.kp[f, :cnt].cpu().numpy(), rkp), (tag, f)
    assert np.array_equal(k.des[f, :cnt].cpu().numpy(), rdes), (tag, f)
    return cnt


@pytest.mark.parametrize("name", host.CASE_NAMES)
def test_orb_edge_case_matches_oracle(dev, name):
    _, imgs, p = host.case(name)
    k = stages.detect_orb(_t(imgs, dev), p)
    for f in range(len(imgs)):
        cnt = _assert_frame_matches_oracle(k, f, imgs[f], p, name)
        assert (cnt == 0) == (name in host.EMPTY_CASES), (name, f, cnt)


def test_orb_two_batches(dev):
    """700 frames of 512x512 do not fit the launcher's 1 GiB candidate workspace: the
    second batch mixes batch-local indices (candidate lists) with global ones (outputs)."""
    F, H, W, nf = 700, 512, 512, 50
    # kcmc_orb_detect's batch size, restated.  If the 1 GiB budget or the per-frame workspace
    # changes so that F frames fit one batch, this test no longer covers the loop: the
    # assertion below then fails, and F must grow.
    ntiles = -(-W // 64) * -(-H // 16)
    slots = ntiles * (64 * 16 // 4)
    per_frame = 2 * slots * (8 + 4) + ntiles * 2 * 4 + 4
    batch = min(max(1, min(F, (1 << 30) // per_frame)), 65535)
    assert batch == 681 and F >= batch + 2
    base = _t(host._texture_u8(np.random.default_rng(21), H, W), dev)
    frames = torch.stack([torch.roll(base, (37 * f, 53 * f), (0, 1)) for f in range(F)])
    twin = batch + 5
    frames[twin] = frames[3]  # the same content in both batches
    p = orb.OrbParams(n_features=nf)
    k = stages.detect_orb(frames, p)
    cnt = k.count.cpu().numpy()
    assert (cnt == nf).all()  # every row of kp / des is written: whole tensors compare below
    assert np.array_equal(frames[batch + 1].cpu().numpy(), np.roll(base.cpu().numpy(), (37 * (batch + 1), 53 * (batch + 1)), (0, 1)))
    for f in (0, batch - 1, batch, batch + 1, F - 1):
        _assert_frame_matches_oracle(k, f, frames[f].cpu().numpy(), p, "two_batches")
    tail = stages.detect_orb(frames[batch:], p)  # the second batch's frames as a first batch
    assert torch.equal(tail.count, k.count[batch:])
    assert torch.equal(tail.kp, k.kp[batch:]) and torch.equal(tail.des, k.des[batch:])
    assert torch.equal(k.kp[twin], k.kp[3]) and torch.equal(k.des[twin], k.des[3])


def test_orb_zero_features(dev):
    """n_features == 0 needs only the counts: the empty kp / des tensors reach the C ABI as
    NULL, which must not be an error."""
    imgs = host.edges_img()[None]
    k = stages.detect_orb(_t(imgs, dev), orb.OrbParams(n_features=0))
    assert k.kp.shape == (1, 0, 2) and k.des.shape == (1, 0, 32)
    assert k.count.cpu().numpy().tolist() == [0]
    assert len(host.detect_oracle(imgs[0], orb.OrbParams(n_features=0))[0]) == 0


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_orb_misaligned_stack(dev, offset):
    """A contiguous [F, H, W] view that starts at an odd byte of its storage: W % 4 == 0
    alone would choose 4-byte loads at misaligned addresses; the launcher must take the
    byte paths instead, with the same result."""
    imgs = host.geometry_imgs(49, 128)
    F, H, W = imgs.shape
    buf = torch.zeros(offset + F * H * W + 8, dtype=torch.uint8, device=dev)
    view = buf[offset:offset + F * H * W].view(F, H, W)
    view.copy_(_t(imgs, dev))
    assert view.is_contiguous() and view.data_ptr() % 4 == offset and W % 4 == 0
    p = orb.OrbParams()
    k = stages.detect_orb(view, p)
    for f in range(F):
        assert _assert_frame_matches_oracle(k, f, imgs[f], p, "misaligned") > 0
    aligned = stages.detect_orb(_t(imgs, dev), p)
    assert torch.equal(aligned.count, k.count)
    for f in range(F):  # the rows past count[f] are unwritten
        n = int(k.count[f].cpu())
        assert torch.equal(aligned.kp[f, :n], k.kp[f, :n]) and torch.equal(aligned.des[f, :n], k.des[f, :n])


def test_orb_argument_errors(dev):
    """Rejected before any kernel is launched."""
    t = _t(host.edges_img()[None], dev)
    with pytest.raises(ValueError, match="edge"):
        stages.detect_orb(t, orb.OrbParams(edge=15))
    for thr in (-1, 256):
        with pytest.raises(ValueError, match="threshold"):
            stages.detect_orb(t, orb.OrbParams(fast_threshold=thr))
    wide = torch.zeros((1, 33, 65536), dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.KcmcError, match="65536"):
        stages.detect_orb(wide, orb.OrbParams(n_features=1))
    for bad in (t[:, :, ::2], t.transpose(1, 2)):
        assert not bad.is_contiguous()
        with pytest.raises(ValueError, match="contiguous"):
            stages.detect_orb(bad)
    torch.cuda.synchronize()
