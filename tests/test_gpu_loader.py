"""core/loader.TrainDataLoader on the GPU. Small frames (48x64, K scaled to match, two ellipsoid classes, M = 5 observed frames,
R = 3 rendered poses each, batches of 4: three batches per epoch, three pairs dropped) against the chain written out by hand:
ingest, sample_rendered_poses with ids e·15 + p, render_batch, get_data_pair_train_batch. One test at full size (fc6 fixes
480x640): fit over the loader equals a hand loop of train_step over a second loader with the same seed, bit for bit."""
import numpy as np
import pytest

import test_gpu_fit as tf
from mx_deepim_amd import synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.core.loader import TrainDataLoader
from mx_deepim_amd.core.module import MutableModule
from mx_deepim_amd.lib.pair_matching import data_pair
from mx_deepim_amd.lib.pair_matching.pose_sampler import sample_rendered_poses
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py
from mx_deepim_amd.lib.utils import image as dimage
from mx_deepim_amd.lib.utils.mask_dilate import mask_dilate_batch
from mx_deepim_amd.runtime import DeviceArray, lib

pytestmark = pytest.mark.gpu
H, W, M, R, BS, SEED = 48, 64, 5, 3, 4, 21
K_SMALL = (np.diag([0.1, 0.1, 1.0]) @ synthetic.K_LINEMOD.astype(np.float64)).astype(np.float32)
NOISE = {"border": 4.0}             # the toolkit's 16 px belong to a 640x480 frame
AXES = ([0.05, 0.04, 0.035], [0.03, 0.06, 0.04])
N_POINTS = 16


def _config(mask_dilate=False):
    cfg = default_config()
    cfg.SCALES = [(H, W)]
    cfg.dataset.INTRINSIC_MATRIX = K_SMALL
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = True
    cfg.network.INPUT_MASK = cfg.network.INPUT_DEPTH = True
    cfg.TRAIN.MASK_DILATE = mask_dilate
    return cfg


def _observed_from_renders(ctx, rm, poses, cls):
    """Observed frames made by rendering the ground-truth poses and quantising them as a camera would: uint8 BGR, uint16
    millimetres, uint8 label maps holding mask_idx = class + 1."""
    image, depth = rm.render_batch(ctx.array(cls, dtype=np.int32), ctx.array(poses))
    rgb = image.asnumpy() + rm.pixel_means.reshape(1, 3, 1, 1)
    bgr = np.ascontiguousarray(np.clip(np.rint(rgb), 0, 255).astype(np.uint8)[:, ::-1].transpose(0, 2, 3, 1))
    d16 = np.rint(depth.asnumpy()[:, 0] * 1000.0).astype(np.uint16)
    mask_idx = (np.asarray(cls) + 1).astype(np.int32)
    labels = ((d16 > 0) * mask_idx[:, None, None]).astype(np.uint8)
    assert (labels.reshape(len(cls), -1).max(1) > 0).all()         # every object is in its frame
    return {"image_observed": bgr, "depth_gt_observed": d16, "depth_observed": d16.copy(), "mask_gt_observed": labels,
            "mask_idx": mask_idx, "pose_observed": poses, "class_index": np.asarray(cls, np.int32)}


@pytest.fixture(scope="module")
def world(ctx):
    cfg = _config()
    rng = np.random.default_rng(77)
    meshes = {}
    for name, axes in zip("ab", AXES):
        meshes[name] = synthetic.ellipsoid_mesh(axes, 12, 24)
        meshes[name].pop("uv")
    means_rgb = dimage._means_rgb(cfg)
    rm = Render_Py("unused", ["a", "b"], K_SMALL, W, H, meshes=meshes, ctx=ctx, pixel_means=np.asarray(means_rgb, np.float32))
    poses = np.zeros((M, 3, 4), np.float32)
    for i in range(M):
        poses[i, :, :3] = synthetic.random_rotation(rng)
        poses[i, :, 3] = [rng.uniform(-0.05, 0.05), rng.uniform(-0.04, 0.04), rng.uniform(0.5, 0.7)]
    cls = np.array([0, 1, 1, 0, 1], np.int32)
    observed = _observed_from_renders(ctx, rm, poses, cls)
    points = {c: (synthetic.sample_model_points(rng, AXES[c], N_POINTS), np.ones((3, N_POINTS), np.float32)) for c in (0, 1)}
    return cfg, rm, observed, points


def _loader(world, cfg=None, **kw):
    cfg0, rm, observed, points = world
    args = dict(batch_size=BS, seed=SEED, num_rendered_per_observed=R, points=points, noise=NOISE)
    args.update(kw)
    return TrainDataLoader(observed, cfg or cfg0, rm, **args)


def _hand_batch(ctx, world, cfg, pairs, ids):
    """The chain the loader is specified as, written out: -> (data, label, attempts)."""
    _cfg, rm, obs, points = world
    m = np.asarray(pairs) // R
    frames = {"depth_gt_observed": obs["depth_gt_observed"][m], "depth_observed": obs["depth_observed"][m],
              "mask_gt_observed": obs["mask_gt_observed"][m], "mask_idx": obs["mask_idx"][m]}
    batch = {"image_observed": dimage.transform_batch(ctx, ctx.array(obs["image_observed"][m], dtype=np.uint8), dimage._means_rgb(cfg)),
             "depth_gt_observed": dimage._depth(ctx, frames, "depth_gt_observed", cfg),
             "depth_observed": dimage._depth(ctx, frames, "depth_observed", cfg),
             "mask_gt_observed": dimage.label_mask(ctx, frames, "mask_gt_observed"),
             "pose_observed": ctx.array(obs["pose_observed"][m]), "class_index": ctx.array(obs["class_index"][m], dtype=np.int32)}
    batch["pose_rendered"], attempts = sample_rendered_poses(batch["pose_observed"], K_SMALL, W, H, SEED, draw_ids=np.asarray(ids),
                                                             noise=NOISE)
    batch["image_rendered"], batch["depth_rendered"] = rm.render_batch(batch["class_index"], batch["pose_rendered"])
    if cfg.TRAIN.MASK_DILATE:
        thick = ctx.empty((len(m), 4), np.int32)
        lib.deepim_sample_mask_dilate(ctx.handle, thick, 10, SEED, 0, ctx.array(np.asarray(ids), dtype=np.uint64), len(m))
        batch["mask_dilate_thickness"] = thick
    batch["point_cloud_model"] = ctx.array(np.stack([points[int(c)][0] for c in obs["class_index"][m]]))
    batch["point_cloud_weights"] = ctx.array(np.stack([points[int(c)][1] for c in obs["class_index"][m]]))
    out = data_pair.get_data_pair_train_batch(batch, cfg)
    return out["data"], out["label"], attempts.asnumpy()


def _host(d):
    return {k: v.asnumpy() for k, v in d.items()}


def _same(a, b):
    assert set(a) == set(b)
    for k in sorted(a):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)


def _epochs(loader, n):
    """[[(data, label) on the host per batch] per epoch]"""
    out = []
    for _ in range(n):
        out.append([(_host(d), _host(l)) for d, l in loader])
        loader.reset()
    return out


@pytest.fixture(scope="module")
def two_epochs(ctx, world):
    loader = _loader(world)
    assert len(loader) == 3 and loader.dropped == 3 and loader.batch_size == BS
    got = _epochs(loader, 2)
    return got, loader.stats()


def test_batches_equal_the_hand_written_chain(ctx, world, two_epochs):
    got, stats = two_epochs
    cfg = world[0]
    attempts = []
    for e in range(2):
        assert len(got[e]) == 3
        for nb, (data, label) in enumerate(got[e]):
            pairs = np.arange(nb * BS, (nb + 1) * BS)
            want_data, want_label, a = _hand_batch(ctx, world, cfg, pairs, e * M * R + pairs)
            attempts.append(a)
            assert set(data) == {"image_observed", "image_rendered", "depth_gt_observed", "class_index", "src_pose", "tgt_pose",
                                 "depth_observed", "depth_rendered", "mask_observed", "mask_rendered"}
            assert set(label) == {"rot", "trans", "mask_gt_observed", "flow", "flow_weights", "point_cloud_model",
                                  "point_cloud_weights", "point_cloud_observed"}
            _same(data, _host(want_data))
            _same(label, _host(want_label))
            assert data["image_rendered"].shape == (BS, 3, H, W) and np.count_nonzero(data["depth_rendered"]) > 0
            assert np.count_nonzero(label["flow_weights"]) > 0
    attempts = np.concatenate(attempts)
    # stats(): the sums of the attempts arrays read in the hand chain
    assert stats == {"pairs": 24, "attempts": int(attempts.sum()), "exhausted": int((attempts == 0).sum())}
    assert stats["attempts"] >= 24 - stats["exhausted"]


def test_epochs_and_seeds(ctx, world, two_epochs):
    got, _stats = two_epochs
    src0 = np.concatenate([d["src_pose"] for d, _l in got[0]])
    src1 = np.concatenate([d["src_pose"] for d, _l in got[1]])
    tgt0 = np.concatenate([d["tgt_pose"] for d, _l in got[0]])
    assert np.array_equal(tgt0, np.concatenate([d["tgt_pose"] for d, _l in got[1]]))
    for p in range(12):
        assert not np.array_equal(src0[p], src1[p]), p          # fresh initial poses every epoch
    again = _epochs(_loader(world), 2)
    for e in range(2):
        for (d0, l0), (d1, l1) in zip(got[e], again[e]):
            _same(d0, d1)
            _same(l0, l1)
    other = _epochs(_loader(world, seed=SEED + 1), 1)
    assert not np.array_equal(np.concatenate([d["src_pose"] for d, _l in other[0]]), src0)
    # shuffle: a permutation of the unshuffled epoch's pairs, each with an unchanged src_pose
    full = _loader(world, batch_size=1)                          # all 15 pairs of epoch 0, in order
    by_pair = np.concatenate([data["src_pose"].asnumpy() for data, _l in full])
    shuffled = _loader(world, shuffle=True)
    order = shuffled.pairs.reshape(-1)
    assert sorted(order.tolist()) != order.tolist() and len(set(order.tolist())) == 12
    got_s = np.concatenate([data["src_pose"].asnumpy() for data, _l in shuffled])
    np.testing.assert_array_equal(got_s.view(np.uint32), by_pair[order].view(np.uint32))
    np.testing.assert_array_equal(by_pair[:12].view(np.uint32), src0.view(np.uint32))
    first = shuffled.pairs.copy()
    shuffled.reset()
    assert not np.array_equal(shuffled.pairs, first) and shuffled.epoch == 1


def test_mask_dilate_uses_the_device_draws(ctx, world):
    cfg = _config(mask_dilate=True)
    loader = _loader(world, cfg=cfg)
    plain = _loader(world)
    changed = 0
    for nb, ((data, label), (pdata, _pl)) in enumerate(zip(loader, plain)):
        pairs = np.arange(nb * BS, (nb + 1) * BS)
        thick = ctx.empty((BS, 4), np.int32)
        lib.deepim_sample_mask_dilate(ctx.handle, thick, 10, SEED, 0, ctx.array(pairs, dtype=np.uint64), BS)
        want = mask_dilate_batch(pdata["mask_observed"], thick).asnumpy()
        np.testing.assert_array_equal(data["mask_observed"].asnumpy(), want)
        changed += int(np.count_nonzero(want != pdata["mask_observed"].asnumpy()))
        want_data, want_label, _a = _hand_batch(ctx, world, cfg, pairs, pairs)
        _same(_host(data), _host(want_data))
        _same(_host(label), _host(want_label))
    assert changed > 0


def test_nothing_is_read_back_inside_an_epoch(ctx, world, monkeypatch):
    loader = _loader(world, cfg=_config(mask_dilate=True))
    reads = []
    real = DeviceArray.asnumpy
    monkeypatch.setattr(DeviceArray, "asnumpy", lambda self: (reads.append(self.nbytes), real(self))[1])
    n = sum(1 for _ in loader)
    loader.reset()
    n += sum(1 for _ in loader)
    assert n == 6 and reads == []
    assert loader.stats()["pairs"] == 24 and reads == [24]                 # one read-back, on demand


def test_refusals(ctx, world):
    cfg, rm, observed, points = world
    dev = dict(observed)
    dev["image_observed"] = ctx.array(observed["image_observed"], dtype=np.uint8)
    with pytest.raises(TypeError, match="device array"):
        TrainDataLoader(dev, cfg, rm, points=points)
    with pytest.raises(NotImplementedError, match="bg_image"):
        TrainDataLoader(dict(observed, bg_image=observed["image_observed"]), cfg, rm, points=points)
    with pytest.raises(NotImplementedError, match="frame_index"):
        TrainDataLoader(dict(observed, frame_index=np.zeros(M, np.int32)), cfg, rm, points=points)
    syn = _config()
    syn.TRAIN.MASK_SYN = True
    with pytest.raises(NotImplementedError, match="MASK_SYN"):
        TrainDataLoader(observed, syn, rm, points=points)
    with pytest.raises(ValueError, match="resize"):
        TrainDataLoader(observed, default_config(), rm, points=points)       # 48x64 frames under SCALES (480, 640)
    with pytest.raises(TypeError, match="uint16"):
        TrainDataLoader(dict(observed, depth_gt_observed=observed["depth_gt_observed"].astype(np.float32)), cfg, rm, points=points)
    with pytest.raises(ValueError, match="points"):
        TrainDataLoader(observed, cfg, rm)


def test_fit_over_the_loader_equals_the_hand_loop_at_full_size(ctx):
    """fc6 fixes 480x640: B = 1, M = 2, TRAIN_ITER_SIZE = 1, one epoch."""
    cfg, net, params, _batches, upd = tf._world(ctx, False, iters=1, n_batches=1)
    rm = upd.render_machine
    rng = np.random.default_rng(5)
    poses = np.stack([synthetic.sample_pose_pair(rng)[0] for _ in range(2)])
    observed = _observed_from_renders(ctx, rm, poses, np.zeros(2, np.int32))
    points = {0: (synthetic.sample_model_points(rng, [0.05, 0.04, 0.035], 3000), np.ones((3, 3000), np.float32))}

    def loader():
        return TrainDataLoader(observed, cfg, rm, batch_size=1, seed=9, points=points)

    first = loader()
    MutableModule(cfg, net, logger=tf._logger("test_gpu_loader.fit", [])).fit(
        first, eval_metric=tf._metrics(cfg), optimizer_params={"learning_rate": tf.LR, "momentum": cfg.TRAIN.momentum, "wd": cfg.TRAIN.wd},
        begin_epoch=0, num_epoch=1, prefix="unused", updater=upd)
    after_fit = tf._state(net)
    assert first.epoch == 1 and first.stats()["pairs"] == 2
    net.bind_train(ctx, 1, params, num_points=3000)
    for data, label in loader():
        net.train_step(data, label, upd, iters=1, lr=tf.LR, wd=cfg.TRAIN.wd, momentum=cfg.TRAIN.momentum)
    tf._assert_same_bytes(after_fit, tf._state(net))
    assert any(k.startswith("mom:") for k in after_fit)
    moved = [k for k, v in params.items() if not np.array_equal(np.asarray(v, np.float32), after_fit["w:" + k])]
    assert moved                                # the two steps really trained
