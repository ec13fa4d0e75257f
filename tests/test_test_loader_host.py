"""core/loader.TestDataLoader without a GPU: the batch plan and its padding, the shuffle, the frames a shared-frame batch uploads,
the observed arrays each configuration asks for, and every refusal — all raised at construction, before a device is touched (the
render machine here is a stand-in whose context is None)."""
import numpy as np
import pytest

from mx_deepim_amd.config import default_config
from mx_deepim_amd.core import loader as L
from mx_deepim_amd.runtime import DeviceArray

H, W, F = 48, 64, 3
CLASSES = ["ape", "cat"]


class Machine(object):
    """What the loader reads of a render machine at construction."""

    def __init__(self, height=H, width=W):
        self.classes, self.height, self.width, self.ctx = list(CLASSES), height, width, None


def _config(**test):
    cfg = default_config()
    cfg.SCALES = [(H, W)]
    for k, v in test.items():
        cfg.TEST[k] = v
    return cfg


def _observed():
    rng = np.random.default_rng(1)
    return {"image_observed": rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8),
            "depth_observed": rng.integers(0, 2000, (F, H, W)).astype(np.uint16),
            "depth_gt_observed": rng.integers(0, 2000, (F, H, W)).astype(np.uint16),
            "mask_gt_observed": rng.integers(0, 3, (F, H, W)).astype(np.uint8),
            "mask_observed": rng.integers(0, 3, (F, H, W)).astype(np.uint8),
            "mask_observed_est": rng.integers(0, 3, (F, H, W)).astype(np.uint8)}


def _pairdb(P=5):
    pose = np.concatenate([np.eye(3), [[0.0], [0.0], [0.6]]], 1).astype(np.float32)
    return [{"frame": [0, 2, 2, 1, 2][p % 5], "gt_class": CLASSES[p % 2], "mask_idx": 1 + p % 2, "pose_observed": pose.copy(),
             "pose_rendered": pose.copy()} for p in range(P)]


def _loader(observed=None, pairdb=None, cfg=None, machine=None, **kw):
    return L.TestDataLoader(_observed() if observed is None else observed, _pairdb() if pairdb is None else pairdb,
                            cfg or _config(), machine or Machine(), **kw)


def test_batch_plan_and_padding():
    ld = _loader(batch_size=2)
    assert ld.size == 5 and len(ld) == 3 and ld.getpad() == 1
    np.testing.assert_array_equal(ld.pairs, [[0, 1], [2, 3], [4, 4]])
    for P, B, n, pad in ((5, 2, 3, 1), (4, 2, 2, 0), (1, 4, 1, 3), (7, 3, 3, 2), (3, 1, 3, 0)):
        pairs, got = L.plan_test_batches(P, B, False, None)
        assert pairs.shape == (n, B) and got == pad
        flat = pairs.reshape(-1)
        np.testing.assert_array_equal(flat[:P], np.arange(P))
        assert (flat[P:] == P - 1).all()
    ld.reset()
    np.testing.assert_array_equal(ld.pairs, [[0, 1], [2, 3], [4, 4]])          # no shuffle: every pass is the same
    with pytest.raises(ValueError, match="batch_size"):
        _loader(batch_size=0)
    with pytest.raises(ValueError, match="empty"):
        _loader(pairdb=[])


def test_shuffle_depends_on_the_seed_only():
    a, b, c = _loader(batch_size=2, shuffle=True, seed=7), _loader(batch_size=3, shuffle=True, seed=7), _loader(batch_size=2, shuffle=True, seed=8)
    passes = []
    for _ in range(3):
        oa, ob, oc = a.pairs.reshape(-1), b.pairs.reshape(-1), c.pairs.reshape(-1)
        np.testing.assert_array_equal(oa[:5], ob[:5])                       # the batch size does not enter the order
        assert sorted(oa[:5].tolist()) == list(range(5)) and oa[5] == oa[4] and a.getpad() == 1 and b.getpad() == 1
        passes.append((oa[:5].tolist(), oc[:5].tolist()))
        for ld in (a, b, c):
            ld.reset()
    want = np.random.RandomState(7)
    assert [p[0] for p in passes] == [want.permutation(5).tolist() for _ in range(3)]
    assert len({tuple(p[0]) for p in passes}) > 1                            # reset() draws a new order
    assert [p[0] for p in passes] != [p[1] for p in passes]                  # another seed, another sequence


def test_frames_of_a_shared_batch_are_uploaded_once():
    rows, index = L.batch_frames([2, 0, 2, 1])
    np.testing.assert_array_equal(rows, [0, 1, 2])
    np.testing.assert_array_equal(index, [2, 0, 2, 1])
    assert index.dtype == np.int32
    rows, index = L.batch_frames([2, 2])
    np.testing.assert_array_equal(rows, [2])
    np.testing.assert_array_equal(index, [0, 0])
    ld = _loader(batch_size=4)
    obs = ld.observed["image_observed"]
    for pairs in ld.pairs:
        rows, index = L.batch_frames(ld.frame[pairs])
        assert len(rows) == len(set(ld.frame[pairs].tolist())) <= len(pairs)
        np.testing.assert_array_equal(obs[rows][index], obs[ld.frame[pairs]])
    np.testing.assert_array_equal(ld.class_index, [0, 1, 0, 1, 0])
    np.testing.assert_array_equal(ld.mask_idx, [1, 2, 1, 2, 1])


def test_observed_keys_follow_the_configuration():
    cfg = _config()
    assert L.observed_keys_of_test(cfg) == ["image_observed"]                 # box_rendered, no depth, FAST_TEST
    for init, key in (("mask_gt_observed", "mask_gt_observed"), ("box_gt_observed", "mask_gt_observed"), ("mask_observed", "mask_observed"),
                      ("box_", "mask_observed")):
        assert L.observed_keys_of_test(_config(INIT_MASK=init)) == ["image_observed", key]
    with pytest.raises(Exception, match="Unknown init mask type"):
        L.observed_keys_of_test(_config(INIT_MASK="nonsense"))
    cfg = _config(FAST_TEST=False)
    assert L.observed_keys_of_test(cfg, ["depth_gt_observed", "depth_observed"]) == ["image_observed", "depth_gt_observed", "mask_gt_observed"]
    assert L.observed_keys_of_test(cfg, ["depth_observed"]) == ["image_observed", "depth_observed", "mask_gt_observed"]
    assert L.observed_keys_of_test(cfg, []) == ["image_observed", "depth_gt_observed", "mask_gt_observed"]
    cfg = _config()
    cfg.network.INPUT_DEPTH = True
    assert L.observed_keys_of_test(cfg) == ["image_observed", "depth_observed"]
    cfg.network.MASK_INPUTS = True
    assert L.observed_keys_of_test(cfg) == ["image_observed", "depth_observed", "mask_observed_est"]
    cfg.dataset.MASK_GT = True
    assert L.observed_keys_of_test(cfg) == ["image_observed", "depth_observed", "mask_gt_observed"]
    cfg.network.INPUT_MASK = False
    cfg.TEST.INIT_MASK = "mask_observed"                                       # not read without INPUT_MASK
    assert L.observed_keys_of_test(cfg) == ["image_observed", "depth_observed", "mask_gt_observed"]


def test_missing_observed_arrays_are_named_at_construction():
    def without(*keys):
        return {k: v for k, v in _observed().items() if k not in keys}

    with pytest.raises(KeyError, match="image_observed"):
        _loader(observed=without("image_observed"))
    with pytest.raises(KeyError, match="mask_gt_observed"):
        _loader(observed=without("mask_gt_observed"), cfg=_config(INIT_MASK="box_gt_observed"))
    with pytest.raises(KeyError, match="'mask_observed'"):
        _loader(observed=without("mask_observed"), cfg=_config(INIT_MASK="mask_observed"))
    with pytest.raises(KeyError, match="mask_gt_observed"):
        _loader(observed=without("mask_gt_observed"), cfg=_config(FAST_TEST=False))
    with pytest.raises(KeyError, match="depth_gt_observed"):
        _loader(observed=without("depth_gt_observed", "depth_observed"), cfg=_config(FAST_TEST=False))
    assert _loader(observed=without("depth_gt_observed"), cfg=_config(FAST_TEST=False)).keys == ["image_observed", "depth_observed", "mask_gt_observed"]
    cfg = _config()
    cfg.network.INPUT_DEPTH = True
    with pytest.raises(KeyError, match="depth_observed"):
        _loader(observed=without("depth_observed"), cfg=cfg)
    assert _loader(observed=without("depth_gt_observed", "mask_gt_observed", "mask_observed", "mask_observed_est", "depth_observed")).keys == ["image_observed"]


def test_refusals_need_no_device():
    obs = _observed()
    dev = dict(obs, image_observed=DeviceArray(None, (F, H, W, 3), np.uint8, ptr=256))     # a view: nothing is allocated
    with pytest.raises(TypeError, match="device array"):
        _loader(observed=dev)
    with pytest.raises(TypeError, match="uint8"):
        _loader(observed=dict(obs, image_observed=obs["image_observed"].astype(np.float32)))
    with pytest.raises(TypeError, match="uint16"):
        _loader(observed=dict(obs, depth_gt_observed=obs["depth_gt_observed"].astype(np.float32)), cfg=_config(FAST_TEST=False))
    with pytest.raises(ValueError, match="SCALES"):
        _loader(observed=dict(obs, image_observed=obs["image_observed"][:, :40]))
    with pytest.raises(ValueError, match="mask_gt_observed"):
        _loader(observed=dict(obs, mask_gt_observed=obs["mask_gt_observed"][:2]), cfg=_config(INIT_MASK="mask_gt_observed"))
    with pytest.raises(ValueError, match="render machine draws 24x32"):
        _loader(machine=Machine(24, 32))
    for bad in (F, -1):
        db = _pairdb()
        db[3]["frame"] = bad
        with pytest.raises(ValueError, match="pair 3 looks at frame %d" % bad):
            _loader(pairdb=db)
    db = _pairdb()
    db[2]["gt_class"] = "dog"
    with pytest.raises(ValueError, match="pair 2 is of class 'dog'"):
        _loader(pairdb=db)
    db = _pairdb()
    del db[1]["pose_rendered"]
    with pytest.raises(KeyError, match="pair 1 carries no 'pose_rendered'"):
        _loader(pairdb=db)
    db = _pairdb()
    db[4]["pose_rendered"] = np.eye(4)
    with pytest.raises(ValueError, match="pair 4"):
        _loader(pairdb=db)
    cfg = _config()
    cfg.network.INPUT_MASK = False
    with pytest.raises(NotImplementedError, match="shared_frames=False"):
        _loader(cfg=cfg)
    assert _loader(cfg=cfg, shared_frames=False).size == 5                    # per pair, the mask-less configuration is served
