"""Shared by tests/test_dense_levels_cpu.py and tests/test_gpu_dense_levels.py: the shapes of the dense-where-it-fits tests, the index
array formed by the rule itself, and the model's oracle values from oracle.gngf_oracle's own pieces.  No test lives here."""
import numpy as np

from oracle import gngf_oracle as orc

N_MIN, N_MAX, L = 8, 32, 4
N_LS = orc.level_resolutions(N_MIN, N_MAX, L)          # 8, 12, 20, 32


def dense_hash_idx(x, n_ls, T):
    """(P,L,4) int64 by the rule: the oracle's hash, and in a level with (N + 2)^2 <= T row gy (N + 2) + gx of the corner
    (gx on input dim 0; clamped to the grid, which coordinates in [0, 1] never need)"""
    _, grid = orc.scale_to_grid(x, n_ls)
    gi = grid.astype(np.int32)                                   # (P,2,L,4)
    idx = orc.spatial_hash(gi, T)
    for l, n in enumerate(int(v) for v in n_ls):
        gw = n + 2
        if gw * gw <= T:
            gx, gy = np.clip(gi[:, 0, l], 0, gw - 1).astype(np.int64), np.clip(gi[:, 1, l], 0, gw - 1).astype(np.int64)
            idx[:, l] = gy * gw + gx
    return idx


def cfg(T, F=2, fp16=False):
    from test_gpu_render import cfg as _render_cfg
    return _render_cfg(dict(L=L, F=F, n_min=N_MIN, n_max=N_MAX), "hash", T, fp16=fp16)


def oracle_model(p, x, T, target=None):
    idx = dense_hash_idx(x, N_LS, T)
    enc = orc.bilinear_forward(x, N_LS, orc.encoding_forward(p["tables"], idx))
    rgb = orc.decoder_forward(enc, p["dec_w"], p["dec_b"])
    if target is None:
        return idx, rgb
    gy = (2.0 / rgb.size) * (rgb.astype(np.float64) - target.astype(np.float64))           # d MSELoss / d rgb
    denc, dWs, dbs = orc.decoder_backward(enc, p["dec_w"], p["dec_b"], gy.astype(np.float32))
    dt, _ = orc.encoding_backward(p["tables"], idx, None, True, orc.bilinear_backward(x, N_LS, denc, p["tables"].shape[2]))
    return idx, rgb, dt, dWs, dbs
