#!/usr/bin/env python
"""Golden vectors of the test loop's flow EPE, produced by running the REFERENCE'S OWN deepim/core/tester.py.

Runs only in the build container (needs /root/reference):  python tests/golden/make_flow_epe_golden.py
Writes tests/golden/flow_epe_golden.npz (committed; data only).  TEST INFRASTRUCTURE ONLY.

Imported UNMODIFIED from /root/reference: deepim/core/tester.py (`par_generate_gt` :530-569, `calc_EPE_one_pair` :572-589) with
what it pulls in (lib/pair_matching/flow.py, lib/utils/projection.py, lib/utils/image.py `resize`, …). Modules that are not
installed, or that only the parts not driven here need, are stand-ins put into sys.modules first (make_ingest_golden.py is the
precedent): cv2 (`imread` hands back in-memory arrays keyed by path, `resize` asserts a scale of 1), mxnet (`cpu`), termcolor,
tqdm, lib.render_glumpy.render_py_multi, lib.utils.PrefetchingIter and deepim.core.module. Three names NumPy 2 removed are
injected before import.

Per tag (frames of 6x12 with B = 2, 7x13 with B = 3) and per STANDARD_FLOW_REP setting the file holds the decoded frames
(uint16 depths, uint8 label map, mask_idx), the poses, K, the fp32 prediction, and what the reference made of them: the float64
ground-truth flow and visible map of par_generate_gt and the six values of calc_EPE_one_pair per pair — once with
"depth_gt_observed" in the pair record and once without (then :545-547 read "depth_observed").

Inputs. K and the poses are dyadic rationals of a few bits, so K·se3_mul(tgt, se3_inverse(src)) is exact in float32 whatever
order (or fused multiply-add) a BLAS uses: the transform the reference builds is the transform the device builds, bit for bit,
and what is compared is the per-pixel float64 arithmetic and the sums. The observed depth is built from the rendered depth's own
projection, then pushed out of the 3 mm threshold, zeroed or relabelled on chosen pixels; main() asserts that no pixel sits
within 1e-7 of a decision (the rounding tie of :38-40, the threshold of :49), so `visible` cannot depend on the last bits.
"""
import os
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mx_deepim_amd.config import AttrDict  # noqa: E402

SHAPES = {"a": (2, 6, 12), "b": (3, 7, 13)}
MASK_IDX = {"a": (1, 3), "b": (2, 1, 5)}
DEPTH_FACTOR = 1000
STORE = {}      # path -> array


def install_stand_ins():
    np.float = float
    np.int = int
    np.maximum_sctype = lambda t: np.float64
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_COLOR, cv2.IMREAD_UNCHANGED, cv2.INTER_LINEAR, cv2.INTER_NEAREST = 1, -1, 1, 0

    def imread(path, flags=None):
        return STORE[path].copy()

    def resize(im, dsize, dst=None, fx=None, fy=None, interpolation=None):
        assert dsize is None and fx == 1.0 and fy == 1.0, "stand-in cv2.resize: scale 1 only (%r, %r)" % (fx, fy)
        return im

    cv2.imread, cv2.resize = imread, resize
    sys.modules["cv2"] = cv2
    mx = types.ModuleType("mxnet")
    mx.cpu = lambda *a: "cpu"
    sys.modules["mxnet"] = mx
    tc = types.ModuleType("termcolor")
    tc.colored = lambda s, *a, **k: s
    sys.modules.setdefault("termcolor", tc)
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.ModuleType("tqdm")
    sys.path.insert(0, REF)
    for name, attr in (("lib.render_glumpy.render_py_multi", "Render_Py"), ("lib.utils.PrefetchingIter", "PrefetchingIter"),
                       ("deepim.core.module", "MutableModule")):
        m = types.ModuleType(name)
        setattr(m, attr, type(attr, (object,), {}))
        sys.modules[name] = m


def load_reference():
    install_stand_ins()
    from deepim.core import tester as T
    assert os.path.realpath(T.__file__).startswith(REF)
    return T


def dy(a, q):
    """array of multiples of 1/q"""
    return (np.asarray(a, np.float64) / q).astype(np.float32)


def make_case(tag, rng):
    """frames, poses, K and prediction of one tag; the observed depth is derived from the rendered depth's projection"""
    import flow_epe_emulation as emu
    B, H, W = SHAPES[tag]
    K = np.array([[8, 0, W / 2], [0, 8, H / 2], [0, 0, 1]], np.float32)
    src, tgt = np.zeros((B, 3, 4), np.float32), np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        src[b, :, :3] = dy([[16, -1 - b, 0], [1 + b, 16, 1], [0, -1, 16]], 16)
        src[b, :, 3] = dy([1 - b, 2, 16 + b], 16)
        tgt[b, :, :3] = dy([[16, -2, 1], [2, 16, -b], [-1, b, 16]], 16)
        tgt[b, :, 3] = dy([3 - b, 1 + b, 17], 16)
    dr = np.zeros((B, H, W), np.uint16)
    for b in range(B):
        dr[b, 1:H - 1, 2 + b:W - 2] = rng.integers(900, 1100, (H - 2, W - 4 - b))
        dr[b, 2, 4] = 0                          # a hole inside the object: background there
        dr[b, 0, 0] = 40000                      # projects far outside the frame
    depth_r = dr.astype(np.float32) / np.float32(DEPTH_FACTOR)
    Kinv = emu.inv3(K)
    labels = np.zeros((B, H, W), np.uint8)
    dgt = np.zeros((B, H, W), np.uint16)
    for b in range(B):
        KT = emu.calc_KT(src[b], tgt[b], K)
        # where every rendered pixel lands and at which depth: ask the restatement with an all-pass target
        h, w = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        d = depth_r[b].astype(np.float64)
        Ki, T = Kinv.astype(np.float64).reshape(9), KT.astype(np.float64).reshape(12)
        X, Y, Z = d * (Ki[0] * w + Ki[1] * h + Ki[2]), d * (Ki[3] * w + Ki[4] * h + Ki[5]), d * (Ki[6] * w + Ki[7] * h + Ki[8])
        pz = T[8] * X + T[9] * Y + T[10] * Z + T[11] + 1e-15
        pw, ph = (T[0] * X + T[1] * Y + T[2] * Z + T[3]) / pz, (T[4] * X + T[5] * Y + T[6] * Z + T[7]) / pz
        for y in range(H):
            for x in range(W):
                if dr[b, y, x] == 0:
                    continue
                xr, yr = int(np.rint(pw[y, x])), int(np.rint(ph[y, x]))
                if 0 <= xr < W and 0 <= yr < H and dgt[b, yr, xr] == 0:
                    dgt[b, yr, xr] = int(np.rint(pz[y, x] * DEPTH_FACTOR))
        labels[b][dgt[b] != 0] = MASK_IDX[tag][b]
        nzy, nzx = np.nonzero(dgt[b])
        pick = rng.permutation(len(nzy))
        for k in pick[:3]:
            dgt[b, nzy[k], nzx[k]] += 10             # 10 mm off: outside the 3 mm threshold
        for k in pick[3:5]:
            labels[b, nzy[k], nzx[k]] = MASK_IDX[tag][b] + 1      # another object's label: zeroed by :556
        for k in pick[5:7]:
            dgt[b, nzy[k], nzx[k]] = 0               # no observed depth: p_valid of :50 fails
    dobs = dgt.copy()
    dobs[:, ::2, ::3] += 7                       # the sensor's depth differs from the ground-truth depth
    est = (rng.standard_normal((B, 2, H, W)) * 2).astype(np.float32)
    est[0, 0, 0, :5] = [2049.0, 1e-8, 1000.3, -2051.0, 6e-8]         # fp16 ties, subnormals, a value fp16 cannot hold
    est[-1, 1, H - 1, W - 3:] = [0.33337402, -0.1, 3.0e-5]          # a tie between two fp16 values, small values
    return {"K": K, "pose_rendered": src, "pose_observed": tgt, "depth_rendered": dr, "depth_gt_observed": dgt,
            "depth_observed": dobs, "mask_gt_observed": labels, "mask_idx": np.array(MASK_IDX[tag], np.int32), "flow_est": est}


def make_config(tag, case, standard_rep):
    B, H, W = SHAPES[tag]
    cfg = AttrDict()
    cfg.SCALES = [(H, W)]
    cfg.network = AttrDict(PRED_FLOW=True, STANDARD_FLOW_REP=standard_rep)
    cfg.dataset = AttrDict(DEPTH_FACTOR=DEPTH_FACTOR, INTRINSIC_MATRIX=case["K"])
    return cfg


def pair_rec(tag, case, b, tmp, with_gt_depth):
    rec = {"mask_idx": int(case["mask_idx"][b]), "pose_rendered": case["pose_rendered"][b],
           "pose_observed": case["pose_observed"][b]}
    keys = ["depth_rendered", "depth_observed", "mask_gt_observed"] + (["depth_gt_observed"] if with_gt_depth else [])
    for key in keys:
        path = os.path.join(tmp, "%s_%s_%d.png" % (tag, key, b))
        open(path, "w").close()
        STORE[path] = case[key][b]
        rec[key] = path
    return rec


def assert_decisions_are_clear(case, flow_gt_vis, with_gt_depth):
    """no pixel within 1e-7 of the rounding tie or of the threshold, in the restatement's own float64 numbers"""
    import flow_epe_emulation as emu
    K, Kinv = case["K"], emu.inv3(case["K"])
    B, H, W = case["depth_rendered"].shape
    for b in range(B):
        ds = case["depth_rendered"][b].astype(np.float32) / np.float32(DEPTH_FACTOR)
        dt = case["depth_gt_observed" if with_gt_depth else "depth_observed"][b].astype(np.float32) / np.float32(DEPTH_FACTOR)
        dt[case["mask_gt_observed"][b] != case["mask_idx"][b]] = 0
        KT = emu.calc_KT(case["pose_rendered"][b], case["pose_observed"][b], K)
        h, w = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        d = ds.astype(np.float64)
        Ki, T = Kinv.astype(np.float64).reshape(9), KT.astype(np.float64).reshape(12)
        X, Y, Z = d * (Ki[0] * w + Ki[1] * h + Ki[2]), d * (Ki[3] * w + Ki[4] * h + Ki[5]), d * (Ki[6] * w + Ki[7] * h + Ki[8])
        pz = T[8] * X + T[9] * Y + T[10] * Z + T[11] + 1e-15
        pw, ph = (T[0] * X + T[1] * Y + T[2] * Z + T[3]) / pz, (T[4] * X + T[5] * Y + T[6] * Z + T[7]) / pz
        nz = ds != 0
        for v in (pw, ph):
            assert np.abs(np.abs(v[nz] - np.floor(v[nz])) - 0.5).min() > 1e-7, "a projection sits on a rounding tie"
        xr, yr = np.clip(np.rint(pw), 0, W - 1).astype(int), np.clip(np.rint(ph), 0, H - 1).astype(int)
        gap = np.abs(np.abs(dt[yr, xr].astype(np.float64) - pz) - 3e-3)
        assert gap[nz].min() > 1e-7, "a depth difference sits on the threshold"
        _, _, vis = emu.calc_flow_core(ds, dt, KT, Kinv, 3e-3)
        assert np.array_equal(vis, flow_gt_vis[b] == 1), "the restatement's visible differs from the reference's"


def main():
    T = load_reference()
    tmp = tempfile.mkdtemp()
    out = {}
    for tag in sorted(SHAPES):
        B, H, W = SHAPES[tag]
        case = make_case(tag, np.random.default_rng(2000 + ord(tag)))
        for k, v in case.items():
            out["%s_%s" % (tag, k)] = v
        for rep in (False, True):
            cfg = make_config(tag, case, rep)
            for with_gt in (True, False):
                name = "%s_ref_%s_%s" % (tag, "std" if rep else "old", "gt" if with_gt else "nogt")
                rows, flows, viss = [], [], []
                for b in range(B):
                    gt = T.par_generate_gt(cfg, pair_rec(tag, case, b, tmp, with_gt))
                    pred = {"flow": case["flow_est"][b].transpose(1, 2, 0).astype("float16")}     # tester.py:350-352
                    d = T.calc_EPE_one_pair(pred, gt, "flow")
                    for k in ("epe_all", "epe_viz", "epe_vizbg"):
                        assert np.asarray(d[k]).dtype == np.float64
                    rows.append([d["epe_all"], d["num_all"], d["epe_viz"], d["num_viz"], d["epe_vizbg"], d["num_vizbg"]])
                    flows.append(gt["flow"][0])
                    viss.append(gt["flow"][1])
                    assert gt["flow"][0].dtype == np.float64
                    assert np.array_equal(gt["flow"][2], (gt["flow"][1] == 0) & (case["depth_rendered"][b] == 0))
                out[name + "_rows"] = np.array(rows, np.float64)
                out[name + "_flow_gt"] = np.stack(flows)
                out[name + "_visible"] = np.stack(viss).astype(np.uint8)
                assert_decisions_are_clear(case, np.stack(viss), with_gt)
                r = out[name + "_rows"]
                assert np.isfinite(r).all() and (r[:, 3] > 4).all() and (r[:, 3] < r[:, 5]).all() and (r[:, 5] < r[:, 1]).all(), r
    path = os.path.join(HERE, "flow_epe_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
