"""Per-pair camera intrinsics: the host side of `deepim_bind_cameras` (include/deepim_hip.h). Pure numpy, no library.

A camera table is a C-contiguous float32 (n,3,3) array, row b the intrinsics of sample b of a batch. The device treats a row as
data (a bad one gives its sample a NaN zoom factor or an empty draw), so a table that comes from the host is checked here, where
the mistake can still be named.
"""
import numpy as np


def validate_cameras(table):
    """-> the table as C-contiguous float32 (n,3,3). ValueError for a wrong shape, a non-finite entry, K[2,2] == 0 or a singular
    matrix (the flow ground truth inverts K; the zoom centre divides by its third row)."""
    t = np.ascontiguousarray(table, dtype=np.float32)
    if t.ndim != 3 or t.shape[1:] != (3, 3) or t.shape[0] < 1:
        raise ValueError("camera table must have shape (n,3,3) with n >= 1, got %s" % (t.shape,))
    for b, K in enumerate(t):
        if not np.isfinite(K).all():
            raise ValueError("camera %d is not finite" % b)
        if K[2, 2] == 0:
            raise ValueError("camera %d has K[2,2] == 0" % b)
        if np.linalg.det(K.astype(np.float64)) == 0:
            raise ValueError("camera %d is singular" % b)
    return t


def camera_table(pair_records, K_default):
    """The (B,3,3) float32 table of a batch of pair records: record b's "K" where it carries one, else `K_default` (the run's
    config.dataset.INTRINSIC_MATRIX). Validated."""
    K_default = np.asarray(K_default, dtype=np.float32).reshape(3, 3)
    rows = [np.asarray(r["K"], dtype=np.float32).reshape(3, 3) if r.get("K") is not None else K_default for r in pair_records]
    return validate_cameras(np.stack(rows))


def has_cameras(pair_records):
    return any(r.get("K") is not None for r in pair_records)
