"""Constants of the hot path, mirroring the reference's config defaults + the shipped YAML
(deepim/config/config.py:11-118, experiments/deepim/cfgs/deepim_flownet_LM_SIXD_v1_ape_RFMx4_8epoch.yaml).
Only the keys the render-and-compare inner loop reads are kept."""
import copy

import numpy as np


class AttrDict(dict):
    """easydict-style attribute access (easydict itself is not a dependency here)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v

    def __deepcopy__(self, memo):
        return AttrDict({k: copy.deepcopy(v, memo) for k, v in self.items()})


# Loss-scale defaults of the fp16 training graph, from the gradient magnitudes of the synthetic batch
FP16_LOSS_SCALE_DEFAULT = 1024.0
FP16_SCALE_WINDOW_DEFAULT = 1000
# Gradient-scale defaults of the split-fp16 training graph (TRAIN.X3_CONV): the largest power of two that keeps every encoder
# layer's scaled max |dz| of the synthetic batches at or below 3750 / 16 (profiles/r12_x3_train.md)
X3_GRAD_SCALE_DEFAULT = 65536.0
X3_SCALE_WINDOW_DEFAULT = 1000


def default_config():
    cfg = AttrDict()
    cfg.default = AttrDict(frequent=1000)   # config.py:21 — Speedometer's interval (train.py:241 passes args.frequent)
    cfg.dataset = AttrDict(
        INTRINSIC_MATRIX=np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], dtype=np.float32),
        NORMALIZE_FLOW=20.0,
        NORMALIZE_3D_POINT=0.1,
        trans_means=np.array([0.0, 0.0, 0.0]),
        trans_stds=np.array([1.0, 1.0, 1.0]),
        DEPTH_FACTOR=1000,   # config.py:55 — raw uint16 depth per metre (lib/utils/image.py)
    )
    cfg.network = AttrDict(
        PIXEL_MEANS=np.array([123.68, 116.779, 103.939], dtype=np.float32),
        INPUT_MASK=True,
        INPUT_DEPTH=False,
        PRED_FLOW=True,
        PRED_MASK=True,
        ROT_TYPE="QUAT",
        ROT_COORD="CAMERA",
        REGRESSOR_NUM=1,
        STANDARD_FLOW_REP=False,
        TRAIN_ITER=True, TRAIN_ITER_SIZE=4,   # yaml :57-58 — refinement iterations inside one training step (module.py:1131-1137)
        X3_CONV=False,     # split-fp16 conv path: fp32-grade accuracy (≈1e-6) on the fp16 matrix cores (not a reference key)
        FP16_CONV=False,   # BASELINE config 5: fp16 conv path (not a reference key; the reference is fp32 only)
        # with FP16_CONV and the decoder in the test graph: decoder + flow / mask predictors in fp16 too (False: fp32 decoder). The
        # training graph ignores it: there the decoder and heads always run in fp32 on the fp16 encoder's activations
        FP16_DECODER=True,
        # with FP16_CONV: the 3x3 stride-1 encoder layers (conv3_1 / conv4_1 / conv5_1 / conv6_1) as fp16 Winograd F(2x2,3x3)
        # (csrc/wino_f16.hip; not a reference key). A second fp16 arithmetic with about 1.5x the direct kernel's per-layer error,
        # 2.25x fewer MFMAs. Test graph only; the x3 and fp32 graphs and the training graph ignore it
        FP16_WINOGRAD=False,
    )
    cfg.train_iter = AttrDict(SE3_PM_LOSS=True, SE3_PM_LOSS_TYPE="L1", LW_PM=0.1, LW_FLOW=0.25, LW_MASK=0.03,
                              NUM_3D_SAMPLE=3000, SE3_PM_SL1_SCALAR=1.0, SE3_DIST_LOSS=False,
                              LW_ROT=0.0, LW_TRANS=0.0, TRANS_LOSS_TYPE="L2", TRANS_SMOOTH_L1_SCALAR=3.0)   # config.py:104-108
    # experiments/deepim/cfgs/deepim_flownet_LM_SIXD_v1_ape_RFMx4_8epoch.yaml:76-92 (keys the label generation reads)
    # (the yaml also sets MASK_DILATE: True — lib/utils/mask_dilate.py: the loader draws the thicknesses with mask_dilate_draws
    # and hands them over in the batch as "mask_dilate_thickness"; the shifted ORs run on the device, deepim_mask_dilate)
    cfg.TRAIN = AttrDict(INIT_MASK="box_gt", FLOW_WEIGHT_TYPE="viz", MASK_DILATE=False,
                         optimizer="sgd", lr=0.0001, momentum=0.975, wd=0.0005,   # config.py:68-77
                         # the keys the training loop reads (core/module.py fit; config.py:69-84): the schedule, the epochs and resume;
                         # VISUALIZE and TENSORBOARD_LOG are refused when set
                         warmup=False, warmup_lr=0, warmup_step=0, begin_epoch=0, end_epoch=0, lr_step="4, 6", RESUME=False,
                         VISUALIZE=False, TENSORBOARD_LOG=False,
                         # mixed-precision training (network.FP16_CONV in the training graph; not reference keys): the initial loss
                         # scale (a power of two) and the number of overflow-free steps after which it doubles
                         FP16_LOSS_SCALE=FP16_LOSS_SCALE_DEFAULT, FP16_SCALE_WINDOW=FP16_SCALE_WINDOW_DEFAULT,
                         # fp32 training on the inference encoder's kernels (not a reference key): channel-blocked
                         # forward activations with fp32 Winograd where the inference path uses it, a backward that reads them in
                         # place, the 3x3 stride-1 data gradients on the Winograd kernels. Same fp32 arithmetic, another summation
                         # order (<= 1e-5 of a layer's range). Ignored with network.FP16_CONV, as network.WINOGRAD_CONV is on the
                         # fp16 inference path; needs the LDS-staged weight gradient (context option "wgrad_lds", the default)
                         WINOGRAD_CONV=False,
                         # split-fp16 training (not a reference key): the x3 encoder forward with a backward on the
                         # fp16 matrix cores at fp32 grade (three MFMAs per product), gradients carried at the power-of-two scale
                         # X3_GRAD_SCALE, which halves on an overflow and doubles after X3_SCALE_WINDOW clean steps. Ignored with
                         # network.FP16_CONV; excludes WINOGRAD_CONV. network.X3_CONV stays a test-graph key
                         X3_CONV=False, X3_GRAD_SCALE=X3_GRAD_SCALE_DEFAULT, X3_SCALE_WINDOW=X3_SCALE_WINDOW_DEFAULT)
    cfg.TEST = AttrDict(test_iter=4, FAST_TEST=True, UPDATE_MASK="box_rendered", INIT_MASK="box_rendered",
                        MASK_DILATE=False,   # yaml :104; image.py:380-381
                        # the other keys the test loop reads (core/tester.py; config.py:93-99): the three below are refused when set
                        VISUALIZE=False, PRECOMPUTED_ICP=False, BEFORE_ICP=False,
                        # not a reference key: refine each batch's final poses against frames["depth_observed"] with the device
                        # depth ICP (lib/pair_matching/depth_icp.py) and report them as "icp" — the device counterpart of the
                        # PRECOMPUTED_ICP row, whose poses the reference reads from files
                        DEPTH_ICP=False)
    cfg.SCALES = [(480, 640)]
    return cfg


ROT_COORD_CODE = {"model": 0, "camera": 1, "camera_new": 2, "naive": 3}
