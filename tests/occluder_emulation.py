"""numpy emulation of deepim_sample_occluders (csrc/sample.hip): the occluders of a synthetic scene, float64 numpy over
pose_sampler_emulation's Philox, uniform, box_muller and below and observed_pose_emulation's quat2mat.  TEST INFRASTRUCTURE ONLY.

Counter layout as in pose_sampler_emulation. Stream 7, attempt 0, word 0 is the count of occluders; stream 7, attempt s is slot
s's class (word 0) and placement (words 1-3: rho, phi, tau); stream 8, attempt s its rotation (four normals). Slot 0 is the
target. The rule is the project's own: the reference has no generator for occluded scenes."""
import numpy as np

import observed_pose_emulation as oemu
import pose_sampler_emulation as emu

TWO_PI = 6.283185307179586


def occluders(seed, ids, target_class, target_pose, classes, diameters, min_occluders=0, max_occluders=2, lateral=(0.2, 0.9),
              toward=(0.5, 1.5)):
    """-> (class (B,S) int32, pose (B,S,3,4) float32, label_value (B,S) int32, n (B) the counts drawn), S = max_occluders + 1.
    diameters: float32 table indexed by class id; lateral / toward reach the device as float32."""
    ids = np.asarray(ids, np.uint64).reshape(-1)
    B, S = ids.size, int(max_occluders) + 1
    target_class = np.asarray(target_class, np.int64).reshape(B)
    target_pose = np.asarray(target_pose, np.float32).reshape(B, 3, 4)
    classes = np.asarray(classes, np.int32).reshape(-1)
    diameters = np.asarray(diameters, np.float32).astype(np.float64).reshape(-1)
    lat = [float(np.float32(v)) for v in lateral]
    tow = [float(np.float32(v)) for v in toward]
    cls, pose = np.full((B, S), -1, np.int32), np.zeros((B, S, 3, 4), np.float32)
    label = np.tile(np.arange(1, S + 1, dtype=np.int32), (B, 1))
    cls[:, 0], pose[:, 0] = target_class, target_pose
    n = np.zeros(B, np.int64)
    if S == 1:
        return cls, pose, label, n
    n = int(min_occluders) + emu.below(emu.draw(seed, ids, 0, 7)[:, 0], int(max_occluders) - int(min_occluders) + 1)
    for s in range(1, S):
        live = np.nonzero(n >= s)[0]
        if live.size == 0:
            continue
        a, r = emu.draw(seed, ids[live], s, 7), emu.draw(seed, ids[live], s, 8)
        u = emu.uniform(a[:, 1:4])
        z0, z1 = emu.box_muller(r[:, 0], r[:, 1])
        z2, z3 = emu.box_muller(r[:, 2], r[:, 3])
        pick = classes[emu.below(a[:, 0], len(classes))]
        for j, b in enumerate(live):
            c = target_class[b]
            d = diameters[c] if 0 <= c < len(diameters) else 0.0
            rho = lat[0] + (lat[1] - lat[0]) * u[j, 0]
            phi = TWO_PI * u[j, 1]
            tau = tow[0] + (tow[1] - tow[0]) * u[j, 2]
            T = target_pose[b].astype(np.float64)
            t = np.array([T[0, 3] + d * (rho * np.cos(phi)), T[1, 3] + d * (rho * np.sin(phi)), T[2, 3] - d * tau])
            if not t[2] > 0.0:
                continue
            z = np.array([z0[j], z1[j], z2[j], z3[j]])
            q = z / np.sqrt(((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]) + z[3] * z[3])
            if q[0] < 0:
                q = -q
            cls[b, s] = pick[j]
            pose[b, s] = np.concatenate([oemu.quat2mat(q), t.reshape(3, 1)], 1).astype(np.float32)
    return cls, pose, label, n
