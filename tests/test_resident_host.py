"""core/resident.ResidentObserved without a GPU: the budget, every refusal of the constructor (raised with ctx = None, before a
device is touched), the rows a batch with synthetic positions reads, that the set and both loaders refuse a bad dict through
one validator, and that a plain dict holding a device array is still refused by both loaders."""
import numpy as np
import pytest

from mx_deepim_amd.config import default_config
from mx_deepim_amd.core import loader as L
from mx_deepim_amd.core.resident import ResidentObserved, batch_rows, check_observed
from mx_deepim_amd.runtime import DeviceArray

H, W, M = 6, 10, 4


class Machine(object):
    """What the loaders read of a render machine at construction."""

    def __init__(self):
        self.classes, self.height, self.width, self.ctx = ["ape", "cat"], H, W, None


def _observed():
    rng = np.random.default_rng(2)
    return {"image_observed": rng.integers(0, 256, (M, H, W, 3), dtype=np.uint8),
            "depth_gt_observed": rng.integers(0, 2000, (M, H, W)).astype(np.uint16),
            "mask_gt_observed": rng.integers(0, 3, (M, H, W)).astype(np.uint8),
            "mask_idx": np.ones(M, np.int32), "class_index": np.zeros(M, np.int32),
            "pose_observed": np.zeros((M, 3, 4), np.float32)}


def test_nbytes_of_a_hand_made_dict():
    obs = _observed()
    frame = H * W * 3 + H * W * 2 + H * W                  # uint8 BGR + uint16 depth + uint8 labels
    assert ResidentObserved.nbytes_of(obs) == M * frame
    assert ResidentObserved.nbytes_of(obs, spare_rows=3) == (M + 3) * frame
    assert ResidentObserved.nbytes_of(obs, keys=["image_observed"], spare_rows=1) == (M + 1) * H * W * 3
    assert ResidentObserved.nbytes_of(obs, ["mask_gt_observed", "image_observed"], 0) == M * H * W * 4
    with pytest.raises(ValueError, match="spare_rows"):
        ResidentObserved.nbytes_of(obs, spare_rows=-1)


def test_every_refusal_comes_before_the_device():
    obs = _observed()
    with pytest.raises(TypeError, match="uint16"):
        ResidentObserved(dict(obs, depth_gt_observed=obs["depth_gt_observed"].astype(np.float32)), None)
    with pytest.raises(TypeError, match="uint8"):
        ResidentObserved(dict(obs, image_observed=obs["image_observed"].astype(np.int16)), None)
    with pytest.raises(ValueError, match="shape"):
        ResidentObserved(dict(obs, mask_gt_observed=obs["mask_gt_observed"][:M - 1]), None)          # unequal M
    with pytest.raises(ValueError, match="shape"):
        ResidentObserved(dict(obs, depth_gt_observed=obs["depth_gt_observed"][:, :, :W - 1]), None)
    with pytest.raises(ValueError, match="shape"):
        ResidentObserved(dict(obs, image_observed=obs["image_observed"][..., :2]), None)
    with pytest.raises(ValueError, match="spare_rows"):
        ResidentObserved(obs, None, spare_rows=-1)
    with pytest.raises(KeyError, match="depth_observed"):
        ResidentObserved(obs, None, keys=["image_observed", "depth_observed"])
    with pytest.raises(ValueError, match="pose_observed"):
        ResidentObserved(dict(obs, pose_observed=np.zeros((M + 1, 3, 4), np.float32)), None)
    with pytest.raises(ValueError, match="one N"):
        ResidentObserved(obs, None, points={0: (np.zeros((3, 5)), np.zeros((3, 5))), 1: (np.zeros((3, 6)), np.zeros((3, 6)))})
    dev = DeviceArray(None, (M, H, W, 3), np.uint8, ptr=4096)          # a view: nothing is allocated
    with pytest.raises(TypeError, match="device array"):
        ResidentObserved(dict(obs, image_observed=dev), None)
    with pytest.raises(ValueError, match="context"):                   # a sound set: only then the device is asked for
        ResidentObserved(obs, None)


def test_rows_of_a_batch_with_synthetic_positions():
    R = 3                                                   # pairs 0..11 are real (frame p // 3), 12.. synthetic
    rows, syn = batch_rows([0, 5, 11, 7], M, R)
    assert rows.dtype == np.int32 and rows.tolist() == [0, 1, 3, 2] and syn.tolist() == []
    rows, syn = batch_rows([12, 4, 14, 13, 10], M, R)       # synthetic pair at position b reads spare row M + b
    assert rows.tolist() == [M + 0, 1, M + 2, M + 3, 3] and syn.tolist() == [0, 2, 3]
    rows, syn = batch_rows([15, 12], M, R)
    assert rows.tolist() == [M, M + 1] and syn.tolist() == [0, 1]
    assert L.batch_rows is batch_rows and L.ResidentObserved is ResidentObserved


def test_one_validator_speaks_through_all_three_constructors():
    """resident.check_observed is the only check of an observed dict: the set and both loaders refuse the same dict with the
    same exception type and the same words, naming the key and what was expected, before a device is touched."""
    obs = _observed()
    keys = ["image_observed", "depth_gt_observed", "mask_gt_observed"]
    cfg = default_config()
    cfg.SCALES = [(H, W)]
    cfg.TEST.FAST_TEST = False                        # the flow EPE: the test loader reads the three arrays too
    assert L.observed_keys_of_test(cfg, list(obs)) == keys and not cfg.network.INPUT_DEPTH
    pose = np.concatenate([np.eye(3), [[0.0], [0.0], [0.6]]], 1).astype(np.float32)
    pairdb = [{"frame": 0, "gt_class": "ape", "mask_idx": 1, "pose_observed": pose, "pose_rendered": pose}]
    constructors = (lambda o: ResidentObserved(o, None, keys=keys), lambda o: L.TrainDataLoader(o, cfg, Machine()),
                    lambda o: L.TestDataLoader(o, pairdb, cfg, Machine()))
    dev = DeviceArray(None, (M, H, W), np.uint8, ptr=4096)          # a view: nothing is allocated
    cases = (
        (dict(obs, depth_gt_observed=obs["depth_gt_observed"].astype(np.float32)), TypeError,
         r"observed\['depth_gt_observed'\] is float32; the decoded uint16 frame is expected"),
        (dict(obs, mask_gt_observed=obs["mask_gt_observed"][:M - 1]), ValueError,                     # unequal M
         r"observed\['mask_gt_observed'\] has shape \(3, 6, 10\); \(4, 6, 10\) expected"),
        (dict(obs, depth_gt_observed=obs["depth_gt_observed"][:, :, :W - 1]), ValueError,
         r"observed\['depth_gt_observed'\] has shape \(4, 6, 9\); \(4, 6, 10\) expected"),
        (dict(obs, image_observed=obs["image_observed"][..., :2]), ValueError,
         r"observed\['image_observed'\] has shape \(4, 6, 10, 2\); \(M,H,W,3\) expected"),
        (dict(obs, mask_gt_observed=dev), TypeError, r"observed\['mask_gt_observed'\] is a device array"),
        ({k: v for k, v in obs.items() if k != "mask_gt_observed"}, KeyError, r"observed carries no 'mask_gt_observed'"),
    )
    for bad, exc, match in cases:
        for construct in constructors:
            with pytest.raises(exc, match=match):
                construct(bad)
    # an array no configuration asked for is not looked at, whatever it holds
    stray = dict(obs, depth_observed=np.zeros((2, 2), np.float32))
    assert list(check_observed(stray, keys)[0]) == keys and L.TestDataLoader(stray, pairdb, cfg, Machine()).keys == keys
    with pytest.raises(ValueError, match="context"):
        ResidentObserved(stray, None, keys=keys)


def test_a_dict_with_a_device_array_is_still_a_type_error_in_both_loaders():
    obs = _observed()
    cfg = default_config()
    cfg.SCALES = [(H, W)]
    dev = DeviceArray(None, (M, H, W, 3), np.uint8, ptr=4096)
    with pytest.raises(TypeError, match="device array"):
        L.TrainDataLoader(dict(obs, image_observed=dev), cfg, Machine())
    pose = np.concatenate([np.eye(3), [[0.0], [0.0], [0.6]]], 1).astype(np.float32)
    pairdb = [{"frame": 0, "gt_class": "ape", "mask_idx": 1, "pose_observed": pose, "pose_rendered": pose}]
    with pytest.raises(TypeError, match="device array"):
        L.TestDataLoader(dict(obs, image_observed=dev), pairdb, cfg, Machine())
