"""CPU: the host side of baking — train.baked_level_offsets (the one statement of the grid layout in Python), argument
validation of train.bake / BakedGrid.render, the gngf_render_grid entry point, data.save_baked / load_baked — and baking
restated in numpy: the vertex grid G = sum_k w table[idx] followed by the four-corner combine is the literal oracle's
function (tests/test_gpu_render.py's expected values), so a render from a baked grid is held to the same oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_gpu_render import ATOL, FIRST, NARROW, RTOL, THREE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resolutions(base):
    from oracle import gngf_oracle as orc
    return [int(n) for n in orc.level_resolutions(base["n_min"], base["n_max"], base["L"])]


def test_entry_point_is_declared_exported_and_bound():
    from collision_handling_in_instantngp_amd import _lib, data, ops, train
    header = open(os.path.join(ROOT, "include", "gngf.h")).read()
    assert re.search(r"\bint\s+gngf_render_grid\s*\(", header)
    assert "#define GNGF_ABI_VERSION 15" in header and _lib.ABI_VERSION == 15
    assert len(_lib.SIGNATURES["gngf_render"]) == 28 and len(_lib.SIGNATURES["gngf_render_grid"]) == 21
    lib = _lib.load()
    assert hasattr(lib, "gngf_render_grid") and lib.gngf_abi_version() == 15
    for fn in (ops.bake_vertex_grid, ops.render_grid, train.bake, train.baked_level_offsets, train.BakedGrid.render,
               train.BakedGrid.render_psnr, data.save_baked, data.load_baked):
        assert callable(fn)
    # rejected arguments come back as hipErrorInvalidValue (1) before anything is launched, so no device is needed and no
    # pointer is followed: every other argument of each call is acceptable (host buffers stand in for device memory)
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15                      # 16-byte aligned
    n_host = (ctypes.c_int32 * 4)(8, 12, 20, 32)
    good = dict(grid=p, n_ls=p, n_ls_host=n_host, W0=p, b0=p, W1=p, b1=p, W2=p, b2=p, rgb=p, img=p, rows=8, cols=8, r0=0, c0=0,
                denom=7.0, L=4, F=2, out_dim=3, leaky=0, stream=None)
    for bad in (dict(F=3), dict(rows=0), dict(denom=0.0), dict(rgb=None, img=None), dict(grid=None), dict(grid=p + 4),
                dict(L=0), dict(L=33), dict(L=4, F=4, out_dim=5), dict(r0=1 << 24)):
        assert lib.gngf_render_grid(*{**good, **bad}.values()) == 1, bad


@pytest.mark.parametrize("base", [FIRST, NARROW, THREE])
def test_baked_level_offsets(base):
    from collision_handling_in_instantngp_amd import train
    n_ls = resolutions(base)
    offsets, vtot = train.baked_level_offsets(n_ls)
    sizes = [(n + 2) ** 2 for n in n_ls]
    assert offsets == [sum(sizes[:l]) for l in range(len(n_ls))] and offsets[0] == 0
    assert vtot == sum(sizes)
    for n in n_ls:
        # the largest corner a coordinate in [0, 1] addresses, in the kernel's arithmetic: floor(fp32(1 * n)) + 1
        hi = int(np.floor(np.float32(1.0) * np.float32(n))) + 1
        assert hi == n + 1 < n + 2
        assert hi * (n + 2) + hi == (n + 2) ** 2 - 1         # the level's last row, still inside it


def test_bake_then_interpolate_is_the_oracle(record_property):
    """NARROW / gngf / T = 256 on 61 x 67.  The oracle evaluates the HPD per pixel corner; baking evaluates it per vertex of
    [0, n_max + 1]^2, sums the K rows in fp32 with k ascending into G (ops.bake_vertex_grid's layout) and reads the four
    corners of a pixel from G.  Same top-K, same blend, same combine, same decoder: the rgb values agree within RTOL, ATOL."""
    import test_gpu_render as tr
    from collision_handling_in_instantngp_amd import train
    from oracle import gngf_oracle as orc
    c = tr.cfg(NARROW, "gngf", 256)
    p = tr.render_params(c)
    n_ls = orc.level_resolutions(c["n_min"], c["n_max"], c["L"])
    L, F, K = c["L"], c["F"], c["K"]
    vstride = c["n_max"] + 2
    gy, gx = np.divmod(np.arange(vstride * vstride), vstride)
    verts = np.stack([gx, gy], axis=1).astype(np.float32)                           # vertex v = gy vstride + gx
    _, tp, ti = orc.hpd_forward(verts, p["hpd_w"], p["hpd_b"], K)
    w = orc.blend_weights(tp, c["blend"])
    offsets, vtot = train.baked_level_offsets([int(n) for n in n_ls])
    G = np.zeros((vtot, F), np.float32)
    for l, n in enumerate(int(n) for n in n_ls):
        yy, xx = np.divmod(np.arange((n + 2) ** 2), n + 2)
        v = yy * vstride + xx
        acc = np.zeros((v.size, F), np.float32)
        for k in range(K):
            acc = (acc + (p["tables"][l][ti[v, k]] * w[v, k, None]).astype(np.float32)).astype(np.float32)
        G[offsets[l]:offsets[l] + v.size] = acc
    x = train.lattice_coordinates(61, 67, 66)
    _, grid = orc.scale_to_grid(x, n_ls)                                            # (P, 2, L, 4): the corners' coordinates
    cx, cy = grid[:, 0].astype(np.int64), grid[:, 1].astype(np.int64)               # (P, L, 4)
    nl = n_ls.astype(np.int64)[None, :, None]
    assert cx.min() >= 0 and cy.min() >= 0 and (cx <= nl + 1).all() and (cy <= nl + 1).all()      # the clamp is idle in [0, 1]^2
    rows = np.asarray(offsets, np.int64)[None, :, None] + cy * (nl + 2) + cx
    feats = np.ascontiguousarray(G[rows].transpose(0, 3, 1, 2))                     # (P, F, L, 4)
    rgb = orc.decoder_forward(orc.bilinear_forward(x, n_ls, feats), p["dec_w"], p["dec_b"], c["leaky"])
    want = tr.want_rgb(c, 61, 67, 66)
    err = np.abs(rgb.astype(np.float64) - want)
    record_property("max_abs_error", float(err.max()))
    print(f"bake-then-interpolate vs the literal oracle: max |error| {err.max():.3e}, "
          f"max error / (ATOL + RTOL |want|) {(err / (ATOL + RTOL * np.abs(want))).max():.3f}")
    np.testing.assert_allclose(rgb, want, rtol=RTOL, atol=ATOL)


def _baked(base=NARROW, C=3, seed=0):
    """a BakedGrid of host tensors (nothing here touches a device)"""
    import torch
    from collision_handling_in_instantngp_amd import train
    n_ls = resolutions(base)
    L, F = base["L"], base["F"]
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g) - 0.5
    return train.BakedGrid(r(train.baked_level_offsets(n_ls)[1], F), [r(64, L * F), r(64), r(64, 64), r(64), r(C, 64), r(C)], n_ls, False)


def test_bake_refuses_what_the_kernel_does_not_hold():
    from collision_handling_in_instantngp_amd import models, train
    from test_render_cpu import _net
    for bad, what in ((_net(True, widths=(64, 32)), "hidden widths"), (_net(False, widths=(64,)), "hidden widths"),
                      (_net(True, L=9, F=8), "hidden widths|at most 64"), (_net(False, L=4, F=3), "1, 2 or 4")):
        with pytest.raises(ValueError, match=what) as e:
            train.bake(bad)
        assert "net(x)" in str(e.value) and str(e.value).startswith("bake()")
    models.should_batchnorm_data = True
    try:
        with pytest.raises(ValueError, match="should_batchnorm_data") as e:
            train.bake(_net(True))
        assert "net(x)" in str(e.value)
    finally:
        models.should_batchnorm_data = False
    with pytest.raises(ValueError, match="out must be a BakedGrid"):
        train.bake(_net(True), out=_baked(THREE))                       # another shape (checked before any device work)
    with pytest.raises(ValueError, match="out must be a BakedGrid"):
        train.bake(_net(True), out=object())


def test_baked_render_refuses_bad_lattices_and_buffers():
    import torch
    baked = _baked()
    # the lattice must lie inside [0, 1]^2 whatever the source of the bake was: the object does not even record it
    assert not hasattr(baked, "mode") and not hasattr(baked, "net")
    for kw in (dict(denom=6), dict(origin=(-1, 0)), dict(origin=(0, 1))):
        with pytest.raises(ValueError, match=r"\[0, 1\]") as e:
            baked.render(**{"rows": 8, "cols": 8, **kw})
        assert "net(x)" in str(e.value)
    for kw in (dict(denom=0), dict(denom=-1.0), dict(rows=0), dict(origin=(1 << 24, 0))):
        with pytest.raises(ValueError):
            baked.render(**{"rows": 8, "cols": 8, **kw})
    with pytest.raises(ValueError, match="ask for rgb"):
        baked.render(8, 8, rgb=False)
    for kw in (dict(out_rgb=torch.empty((64, 3))),                                        # not on the device
               dict(out_image=torch.empty((8, 8, 3), dtype=torch.int32)),
               dict(out_rgb=torch.empty((64, 3), dtype=torch.float64)),
               dict(out_image=torch.empty((8, 8, 3), dtype=torch.int64)),
               dict(out_rgb=torch.empty((63, 3)))):
        with pytest.raises(ValueError, match="out_rgb must be|out_image must be"):
            baked.render(8, 8, **kw)


def test_baked_grid_refuses_tensors_that_do_not_fit():
    import torch
    from collision_handling_in_instantngp_amd import train
    ok = _baked()
    n_ls = ok.n_ls_host
    assert (ok.L, ok.F, ok.out_dim, ok.leaky) == (4, 2, 3, False)
    assert ok.nbytes == 4 * (ok.grid.numel() + sum(t.numel() for t in ok.decoder))
    assert ok.n_ls.dtype == torch.int32 and ok.n_ls.tolist() == n_ls
    with pytest.raises(ValueError, match="grid must be"):
        train.BakedGrid(ok.grid[:-1], ok.decoder, n_ls, False)
    with pytest.raises(ValueError, match="grid must be"):
        train.BakedGrid(ok.grid.double(), ok.decoder, n_ls, False)
    with pytest.raises(ValueError, match="decoder must be"):
        train.BakedGrid(ok.grid, ok.decoder[:5], n_ls, False)
    with pytest.raises(ValueError, match="decoder must be"):
        train.BakedGrid(ok.grid, [ok.decoder[0][:, :-1], *ok.decoder[1:]], n_ls, False)


def test_save_and_load_round_trip(tmp_path):
    import torch
    from collision_handling_in_instantngp_amd import data, train
    baked = _baked(THREE, C=1, seed=3)
    baked.leaky = True
    path = str(tmp_path / "baked.pt")
    data.save_baked(baked, path)
    got = data.load_baked(path, device="cpu")
    assert isinstance(got, train.BakedGrid) and got is not baked
    assert set(train.BakedGrid.FIELDS) == set(data.BAKED_FIELDS)
    for name in train.BakedGrid.FIELDS + ("nbytes",):
        a, b = getattr(baked, name), getattr(got, name)
        if name == "decoder":
            assert len(a) == len(b) == 6 and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))
        elif torch.is_tensor(a):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), name
        else:
            assert type(a) is type(b) and a == b, name
    assert torch.equal(got.n_ls, baked.n_ls) and got.n_ls.dtype == torch.int32
    # a file with another tag, or whose numbers do not fit its tensors, is refused
    state = torch.load(path, weights_only=True)
    assert state["format"] == data.BAKED_FORMAT and state["fields"] == list(data.BAKED_FIELDS)
    torch.save({**state, "format": "something-else/1"}, path)
    with pytest.raises(ValueError, match="not a baked grid"):
        data.load_baked(path, device="cpu")
    torch.save({**state, "F": 2}, path)
    with pytest.raises(ValueError, match="file says"):
        data.load_baked(path, device="cpu")
    torch.save({**state, "grid": state["grid"][:-1]}, path)
    with pytest.raises(ValueError, match="grid must be"):
        data.load_baked(path, device="cpu")
    torch.save([1, 2, 3], path)
    with pytest.raises(ValueError, match="not a baked grid"):
        data.load_baked(path, device="cpu")
