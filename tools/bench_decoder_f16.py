"""A/B of the fp16 decoder: one full refinement iteration of the fp16 conv path with the decoder and both heads in the graph
(FAST_TEST off), network.FP16_DECODER on (NHWC fp16 concats, csrc/decoder_f16.hip) against off (fp32 decoder fed the fp16 encoder's
activations), in the same process, timed with device events, alternating the two. Also decoder() + heads() alone.
usage: bench_decoder_f16.py [B ...]   (default: 8 32). Prints one JSON line per batch."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_deepim_amd import synthetic  # noqa: E402
from mx_deepim_amd.config import default_config  # noqa: E402
from mx_deepim_amd.runtime import Context  # noqa: E402
from mx_deepim_amd.symbols import deepIM_flownet  # noqa: E402

REPS, ROUNDS = 20, 5


def bind(ctx, B, fp16_decoder, params=None):
    cfg = default_config()
    cfg.network.FP16_CONV = True
    cfg.network.FP16_DECODER = fp16_decoder
    cfg.TEST.FAST_TEST = False
    net = deepIM_flownet().get_symbol(cfg)
    params = net.init_weights(cfg, seed=3) if params is None else params
    net.bind(ctx, B, params)
    return net, params


def timed(ctx, fn):
    t = ctx.timer()
    t.start()
    for _ in range(REPS):
        fn()
    t.stop()
    return t.elapsed_ms() / REPS


def main():
    ctx = Context.get(0)
    for B in [int(a) for a in sys.argv[1:]] or [8, 32]:
        d = synthetic.make_batch(B, seed=8, n_frames=1)
        on, params = bind(ctx, B, True)
        off, _ = bind(ctx, B, False, params)
        data = {k: ctx.array(d[k]) for k in ("image_observed", "mask_observed")}
        data.update({k: ctx.array(d[k][0]) for k in ("image_rendered", "mask_rendered", "src_pose")})
        res = {"B": B, "iteration_ms": {"fp16_decoder": [], "fp32_decoder": []}, "decoder_heads_ms": {"fp16_decoder": [], "fp32_decoder": []}}
        nets = (("fp16_decoder", on), ("fp32_decoder", off))
        for _, net in nets:            # warm-up: code objects, plans, scratch
            pose = ctx.empty((B, 3, 4))
            for _ in range(3):
                net.refine_iteration(data, pose)
        ctx.sync()
        for _ in range(ROUNDS):
            for key, net in nets:
                pose = ctx.empty((B, 3, 4))
                res["iteration_ms"][key].append(timed(ctx, lambda: net.refine_iteration(data, pose)))
                res["decoder_heads_ms"][key].append(timed(ctx, lambda: (net.decoder(), net.heads())))
        for group in ("iteration_ms", "decoder_heads_ms"):
            res[group] = {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                          for k, v in res[group].items()}
        res["iteration_speedup"] = res["iteration_ms"]["fp32_decoder"]["median"] / res["iteration_ms"]["fp16_decoder"]["median"]
        flow_on, flow_off = on.act["flow_est"].asnumpy(), off.act["flow_est"].asnumpy()
        res["flow_est_fp16_vs_fp32_decoder_rel"] = float(np.abs(flow_on - flow_off).max() / max(1e-30, np.abs(flow_off).max()))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
