"""Pins the CPU oracle (oracle/edage_np.py, oracle/philox_np.py) against golden vectors captured
from the reference's own EDaGe-PP modules (tests/golden/make_fixtures.py).  CPU only.

Tolerances: the reference and the oracle run the same NumPy here, so most quantities agree
bit for bit; 1e-11 absolute (pixels / world units) absorbs torch.mean-vs-numpy summation order
in the hull centre (Path.py:167).  Integer results (canvas pixel set, hull vertices, isle slice
bounds, accept masks, RNG stream position) must be exact.
"""
import math
import os

import numpy as np
import torch
import pytest

from oracle import edage_np as E
from oracle import philox_np as px

TOL = 1e-11


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _close(a, b, tol=TOL):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size:
        assert float(np.abs(a - b).max()) <= tol, float(np.abs(a - b).max())


# ------------------------------------------------------------------ Philox known answers
def test_philox_random123_kat():
    # Random123 kat_vectors, philox4x32 10 rounds
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = px.philox4x32_10(*ctr, *key)
        assert tuple(int(g) for g in got) == want


def test_philox_streams_are_independent_of_batching():
    a = px.doubles(7, px.STREAM_PATH, 3, 0, 101)
    b = np.concatenate([px.doubles(7, px.STREAM_PATH, 3, 0, 37), px.doubles(7, px.STREAM_PATH, 3, 37, 64)])
    assert (a == b).all() and (a >= 0).all() and (a < 1).all()
    f = px.floats(7, px.STREAM_POCKET, 3, 0, 50)
    g = np.concatenate([px.floats(7, px.STREAM_POCKET, 3, 0, 13), px.floats(7, px.STREAM_POCKET, 3, 13, 37)])
    assert (f == g).all() and f.dtype == np.float32 and (f < 1).all()
    assert not (px.doubles(7, px.STREAM_PATH, 4, 0, 8) == a[:8]).any()


# ------------------------------------------------------------------ G1 PathSeg
@pytest.mark.parametrize("key", ["s0_f0", "s0_f1", "s1_f0", "s1_f1", "s2_f0", "s2_f1", "s7_f0", "s7_f1"])
def test_pathseg_random(golden_dir, key):
    g = _load(golden_dir, "g1_pathseg.npz")
    forced = key.endswith("f1")
    d = g[key + "_draws"]
    d = np.concatenate([[1.0], d]) if forced else d
    r = E.pathseg_random(d, forced)
    _close(r["poly"], g[key + "_poly"], 1e-13)
    _close(r["endpoint"], g[key + "_endpoint"][0], 0)
    _close(r["translation"], g[key + "_translation"], 1e-13)
    _close([r["grad_st"], r["grad_end"]], g[key + "_grad"], 1e-13)
    _close(r["length"], g[key + "_length"][0], 1e-12)
    assert bool(r["straight"]) == bool(g[key + "_straight"][0])


# ------------------------------------------------------------------ G2..G8 one path, every stage
def _cases(golden_dir):
    g = _load(golden_dir, "g2_paths.npz")
    return g, [str(c) for c in g["cases"]]


def _parse(name):
    R = int(name.split("_R")[1].split("_")[0])
    c = int(name.split("_c")[1].split("_")[0])
    return R, c, name.endswith("st1")


def _fixed_layout(compact, straight):
    """golden draws are in the reference's compact consumption order; the oracle takes the fixed
    layout [path flag][seg flag, 1000 samples, end] x 10."""
    full = np.ones(E.DRAWS_PER_PATH)
    full[0] = 0.0 if straight else 1.0
    pos = 0
    for s in range(E.PATHSEGNUM):
        b = 1 + s * E.DRAWS_PER_SEG
        if not straight:
            full[b] = compact[pos]
            pos += 1
        full[b + 1:b + 1 + E.N_FIT] = compact[pos:pos + E.N_FIT]
        pos += E.N_FIT
        full[b + 1 + E.N_FIT] = compact[pos]
        pos += 1
    assert pos == len(compact)
    return full


CASE_NAMES = ["s0_R64_c3_st0", "s1_R64_c3_st0", "s0_R224_c1_st0", "s3_R224_c3_st0", "s0_R256_c3_st0",
              "s1_R256_c3_st0", "s4_R256_c1_st0", "s5_R256_c3_st1", "s6_R128_c3_st0", "s8_R64_c3_st0",
              "s9_R256_c3_st0"]


def test_case_list_matches_fixture(golden_dir):
    g, names = _cases(golden_dir)
    assert names == CASE_NAMES
    # the reference itself never returns for this case (unbounded while loop, Path.py:478)
    assert [str(x) for x in g["reference_nonterminating"]] == ["s2_R64_c1_st0"]


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("mode", ["blas", "plain"])
def test_path_chain(golden_dir, name, mode):
    g, _ = _cases(golden_dir)
    R, c, st = _parse(name)
    G = lambda k: g[f"{name}/{k}"]
    with E.arith(mode):
        path = E.path_generate(_fixed_layout(G("draws"), st))
        assert path["straight"] == st
        _close([s["poly"] for s in path["segs"]], G("seg_poly"), 1e-13)
        _close([s["endpoint"] for s in path["segs"]], G("seg_endpoint"), 0)
        assert [int(s["straight"]) for s in path["segs"]] == G("seg_straight").tolist()
        _close([s["length"] for s in path["segs"]], G("seg_length"), 1e-12)
        _close(path["seg_rot"], G("seg_rotation"))
        _close(path["seg_trans"], G("seg_translation"))
        _close(path["segpoint"], G("segpoint"))
        _close(path["pathpoint"], G("pathpoint_world"))
        _close(path["length"], G("length")[0], 1e-10)

        bnd = E.draw_boundary(path, c)
        _close(bnd["boundarypoint"], G("boundarypoint_world"))
        _close(bnd["up_dir"], G("up_dir"))
        _close(bnd["up_point"], G("up_point"))
        _close(bnd["down_point"], G("down_point"))
        _close(bnd["init"], G("init_boundary"))
        _close(bnd["end"], G("end_boundary"))

        canvas = E.corridor_canvas(path, bnd, R, 50, c)
        assert canvas.shape == (2 * R, 2 * R)
        assert np.array_equal(np.argwhere(canvas), G("canvas_nz"))          # exact pixel set

        hull = E.convexhull(path["pathpoint"], R, 50, order="scipy")
        assert np.array_equal(hull, G("hull_raw"))                          # exact, Qhull order
        canon = E.convexhull(path["pathpoint"], R, 50)
        k = int(np.where((canon == hull[0]).all(1))[0][0])
        assert np.array_equal(np.roll(canon, -k, axis=0), hull)             # same cycle

        nrm = E.space_normalization(path, bnd, canvas, hull, R, 50)
        _close(nrm["rotation"], G("rotation")[0])
        _close(nrm["trans_rc"], G("translation")[::-1], 1e-10)              # stored [t_col, t_row]
        _close(nrm["hull"], G("hull_norm"), 1e-10)
        _close(nrm["segpoint_image"], G("segpoint_image"), 1e-10)
        _close(nrm["pathpoint_image"], G("pathpoint_image"), 1e-10)
        _close(nrm["boundarypoint_image"], G("boundarypoint_image"), 1e-10)
        # the lattice part must be exact
        assert np.array_equal(np.round(nrm["pathpoint_image"] - nrm["trans_rc"]),
                              np.round(G("pathpoint_image") - G("translation")[::-1]))
        assert nrm["space"].shape == (R, R) and nrm["space"].any()

        if not st:
            isles, fl = E.search_isle(nrm["pathpoint_image"], nrm["hull"], R, 50, c)
            assert fl == 0
            assert [list(i) for i in isles] == G("isle_bounds").tolist()    # exact slice bounds
            feed = E._FloatFeed(G("torch_draws"), rotation_draws=int(G("n_rotation_draws")[0]))
            feed.rotation_draw()                                          # Path.py:160-161, ahead of set_obstacles
            obs, fl = E.set_obstacles(nrm["pathpoint_image"], isles, R, 50, c, feed)
            assert fl == 0
            _close(obs, G("obstacles"), 1e-10)


# ------------------------------------------------------------------ G9 boundary_check
def test_boundary_check(golden_dir):
    g = _load(golden_dir, "g9_boundary_check.npz")
    hull, R = g["hull_norm"], int(g["R"][0])
    got = []
    for a, t in zip(g["angles"], g["trans"]):
        ok, h = E.boundary_check(hull, -a, [t[1], t[0]], R)
        got.append(int(ok))
    assert got == g["ok"].tolist()
    assert 0 < sum(got) < len(got)
    for i in range(16):
        _, h = E.boundary_check(hull, -g["angles"][i], [g["trans"][i][1], g["trans"][i][0]], R)
        _close(h, g["hull_out"][i], 1e-10)


# ------------------------------------------------------------------ G10 config 1 end to end
def test_config1_mt_stream_replay(golden_dir):
    """BASELINE config 1: np.random.seed(0); torch.manual_seed(0);
    MapGenerate(10, 64, 50, 5, 20, 3).generate(100) — the oracle, fed by the same global MT19937 /
    torch streams in the reference's order, reproduces every label and obstacle list and leaves
    the numpy stream at exactly the same position."""
    torch = pytest.importorskip("torch")
    g = _load(golden_dir, "g10_config1_R64.npz")
    np.random.seed(0)
    torch.manual_seed(0)
    src = E.MTSource()
    with E.arith("blas"):
        precs = E.generate_paths(src, 10, 64, 50, 3, hull_order="scipy")
        for j, p in enumerate(precs):
            _close(p["hull"], g[f"p{j}/hull_norm"], 1e-10)
            _close(p["segpoint_image"], g[f"p{j}/segpoint_image"], 1e-10)
            _close(p["pathpoint_image"], g[f"p{j}/pathpoint_image"], 1e-10)
            _close(p["obstacles"], g[f"p{j}/obstacles"], 1e-10)
            _close(p["length"], g[f"p{j}/length"][0], 1e-10)
            _close(p["rotation"], g[f"p{j}/rotation"][0])
            assert int(p["straight"]) == int(g[f"p{j}/straight"][0]) and p["flags"] == 0
        maps = E.generate_maps(src, precs, 64, 50, 5, 20, 3, placements=10)
    assert len(maps) == 100
    _close([m["angle"] for m in maps], g["angle"], 0)
    assert np.array_equal(np.array([m["translation"] for m in maps]), g["translation"])
    _close([m["segpoint"] for m in maps], g["segpoint"], 1e-10)
    _close([m["pathpoint"] for m in maps], g["pathpoint"], 1e-10)
    assert [len(m["obstacles"]) for m in maps] == g["n_obs"].tolist()
    _close(np.concatenate([m["obstacles"] for m in maps]), g["obstacles"], 1e-10)
    _close([m["length"] for m in maps], g["problem_length"], 1e-10)
    _close([m["init"] for m in maps], g["problem_init"], 1e-10)
    _close([m["end"] for m in maps], g["problem_end"], 1e-10)
    assert np.array_equal(np.random.random(4), g["np_next_draws"])          # stream position
    assert np.array_equal(np.array([torch.rand(1).item() for _ in range(4)], np.float32), g["torch_next_draws"])   # and torch's
    for m in maps:
        assert m["grid"].shape == (64, 64) and set(np.unique(m["grid"])) <= {0, 128, 255}


# ------------------------------------------------------------------ G12 markers + raster rules
def test_paint_markers(golden_dir):
    g = _load(golden_dir, "g12_init_end.npz")
    ref = g["out"]                                          # [3,64,64], painted with [255,0,0]
    grid = np.full([64, 64], E.GRID_FREE, np.uint8)
    E.paint_markers(grid, g["init"], g["end"])
    assert np.array_equal(grid == E.GRID_MARK, ref[0] == 255)
    assert (ref[1][grid == E.GRID_MARK] == 0).all()


def test_rotate_translate_rules():
    img = np.zeros([9, 9], bool)
    img[2, 6] = True
    assert np.array_equal(E.rotate_nearest(img, 0.0), img)
    r90 = E.rotate_nearest(img, 90.0)                       # counter-clockwise on the display
    assert r90.sum() == 1 and r90[2, 2]
    assert np.array_equal(E.rotate_nearest(E.rotate_nearest(img, 90.0), -90.0), img)
    t = E.translate_nearest(img, 1, 2, 9, 9)                # tx -> columns, ty -> rows
    assert t.sum() == 1 and t[4, 7]
    assert E.translate_nearest(img, 5, 0, 9, 9).sum() == 0  # shifted out: zero fill


# The corridor resample pinned to the primitives torchvision calls.  torchvision is absent here, but its 0.12 tensor path
# (functional.rotate / functional.affine -> functional_tensor._gen_affine_grid -> grid_sample) is a published composition of
# torch ops that ARE importable; the helpers below state that composition with torch itself doing the arithmetic
# (linspace, the float32 division of theta, bmm, grid_sample(nearest, zeros, align_corners=False)).
def _tv_grid_sample(img, matrix):
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32))[None, None]
    h, w = x.shape[-2:]
    theta = torch.tensor(matrix, dtype=torch.float32).reshape(1, 2, 3)
    base = torch.empty(1, h, w, 3, dtype=torch.float32)
    base[..., 0].copy_(torch.linspace(-w * 0.5 + 0.5, w * 0.5 + 0.5 - 1, steps=w))
    base[..., 1].copy_(torch.linspace(-h * 0.5 + 0.5, h * 0.5 + 0.5 - 1, steps=h).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=torch.float32)
    grid = base.view(1, h * w, 3).bmm(rescaled).view(1, h, w, 2)
    return F.grid_sample(x, grid, mode="nearest", padding_mode="zeros", align_corners=False)[0, 0].numpy()


def _tv_rotate(img, angle):            # functional.rotate: matrix for -angle about the centre
    return _tv_grid_sample(img, E.inverse_affine_matrix(-angle, [0.0, 0.0]))


def _tv_random_rotation(img, a):
    """T.RandomRotation(degrees=(a, a))(img) of torchvision 0.12 (transforms.py: get_params returns
    float(torch.empty(1).uniform_(float(degrees[0]), float(degrees[1])).item()), forward calls F.rotate with it) — the
    call the reference makes at Path.py:160-161 and MapGenerate.py:103-104.  The draw is made by torch itself here, so the
    angle is whatever float32 value torch produces for a degenerate range (the global generator is saved and restored)."""
    state = torch.get_rng_state()
    angle = float(torch.empty(1).uniform_(float(a), float(a)).item())
    torch.set_rng_state(state)
    return _tv_rotate(img, angle)


def _tv_translate(img, tx, ty):        # functional.affine(angle=0, translate=[tx, ty], scale=1, shear=0)
    return _tv_grid_sample(img, E.inverse_affine_matrix(0.0, [tx, ty]))


# PyTorch's float32 arithmetic in that composition is not the same on every host: the bmm is MKL's sgemm, whose code path
# follows the CPU, and the oracle (the HIP kernels with it) follows the AVX-512 path.  The tests on random images below therefore
# compare with PyTorch's results recorded on such a host (tests/golden/g17_torch_resample.npz, tests/golden/make_fixtures.py),
# stored as the pixels where they differ from the same composition evaluated in float64 (a few per million).
def _f64_grid_sample(img, matrix):
    """_tv_grid_sample's composition in float64 NumPy: every operation exactly rounded, so the same result on every host
    (grid_sample's nearest mode rounds half to even, as np.rint)."""
    h, w = img.shape
    th = np.asarray(matrix, dtype=np.float64).reshape(2, 3)
    x = np.arange(w, dtype=np.float64)[None, :] + (0.5 - w * 0.5)
    y = np.arange(h, dtype=np.float64)[:, None] + (0.5 - h * 0.5)
    jj, ii = (np.rint(((x * th[k, 0] + y * th[k, 1] + th[k, 2]) / (0.5 * size) + 1.0) * (size / 2) - 0.5).astype(np.int64)
              for k, size in ((0, w), (1, h)))
    return E._gather(np.asarray(img, dtype=np.float32), ii, jj, h, w)


def _f64_rotate(img, angle):
    return _f64_grid_sample(img, E.inverse_affine_matrix(-angle, [0.0, 0.0]))


def _f64_translate(img, tx, ty):
    return _f64_grid_sample(img, E.inverse_affine_matrix(0.0, [tx, ty]))


def _recorded(g17, key, base):
    """PyTorch's result of case `key` as g17 records it: `base`, the float64 evaluation, with PyTorch's values where they differ."""
    out = np.array(base)
    out.reshape(-1)[g17[key + "/at"]] = g17[key + "/val"]
    return out


def _placement_cases(R):
    rng = np.random.default_rng(R)
    for i in range(100 if R == 64 else 34):
        img = rng.random([R, R]) < 0.5
        angle = rng.uniform(-180.0, 180.0)                                  # MapGenerate.py:63
        t = [int(rng.random() ** 2 * R - R / 2), int(rng.random() ** 2 * R - R / 2)]
        yield f"placements_R{R}/{i}", img, angle, t


def _rotation_cases():
    rng = np.random.default_rng(11)
    for i in range(40):
        a = rng.uniform(-180.0, 180.0)
        yield f"rotation/{i}", a, rng.random([512, 512]) < 0.5


def _affine_cases():
    rng = np.random.default_rng(7)
    for (h, w) in ((128, 128), (224, 224), (100, 300), (330, 444), (512, 512)):
        for i in range(4):
            m = E.inverse_affine_matrix(rng.uniform(-180, 180), [rng.uniform(-w / 2, w / 2), rng.uniform(-h / 2, h / 2)])
            yield f"affine_{h}x{w}/{i}", h, w, m


def test_inverse_affine_matrix_closed_forms():
    m = E.inverse_affine_matrix(30.0, [0.0, 0.0])
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    _close(m, [c, s, 0.0, -s, c, 0.0], 0.0)
    _close(E.inverse_affine_matrix(0.0, [3.0, -2.5]), [1.0, 0.0, -3.0, 0.0, 1.0, 2.5], 0.0)


def test_resample_rule_is_torchvisions_tensor_path_on_goldens(golden_dir):
    """Path.py:160-161,175 on the 11 golden corridor canvases at their recorded Rotation / Translation."""
    g = _load(golden_dir, "g2_paths.npz")
    for case in [str(c) for c in g["cases"]]:
        R = int(case.split("_")[1][1:])
        nz = g[case + "/canvas_nz"]
        canvas = np.zeros([2 * R, 2 * R], bool)
        canvas[nz[:, 0], nz[:, 1]] = True
        rot = float(np.asarray(g[case + "/rotation"]).reshape(-1)[0])
        tx, ty = (float(v) for v in g[case + "/translation"])          # Path.Translation = [t_col, t_row]
        want_rot = _tv_random_rotation(canvas, -rot) > 0.5
        got_rot = E.rotate_nearest(canvas, -rot)
        assert np.array_equal(got_rot, want_rot), case
        want = _tv_translate(want_rot, tx, ty)[:R, :R] > 0.5
        assert np.array_equal(E.translate_nearest(got_rot, tx, ty, R, R), want), case
        assert want.sum() > 0


@pytest.mark.parametrize("R", [64, 224, 256])
def test_resample_rule_is_torchvisions_tensor_path_on_placements(golden_dir, R):
    """MapGenerate.py:102-106 on 100 random placements; dense random images, so every pixel of the map is a witness
    (the float64 form of the same map differs from the primitive on ~5 pixels per million of such images)."""
    g17 = _load(golden_dir, "g17_torch_resample.npz")
    for key, img, angle, t in _placement_cases(R):
        # RandomRotation's angle is float32(-angle) (test_rotation_angle_passes_through_float32)
        want = _recorded(g17, key, _f64_translate(_f64_rotate(img, float(np.float32(-angle))), t[0], t[1]) > 0.5)
        got = E.translate_nearest(E.rotate_nearest(img, -angle), float(t[0]), float(t[1]), R, R)
        assert np.array_equal(got, want)


def test_rotation_angle_passes_through_float32(golden_dir):
    """RandomRotation hands F.rotate the angle as a float32 value; rounds 1-4 built the matrix from the float64
    angle (oracle and kernels alike, so no HIP-vs-oracle test could see it).  The draw is float32(a) exactly, the oracle's
    rotate_nearest follows it, and on dense images the two angles give different rasters often enough to tell them apart."""
    g17 = _load(golden_dir, "g17_torch_resample.npz")
    differ = 0
    for key, a, img in _rotation_cases():
        drawn = float(torch.empty(1).uniform_(a, a).item())
        assert drawn == float(np.float32(a))
        want = _recorded(g17, key, _f64_rotate(img, drawn) > 0.5)
        assert np.array_equal(E.rotate_nearest(img, a), want)
        f64_angle = E._gather(img, *E.affine_source_index(512, 512, E.inverse_affine_matrix(-a, [0.0, 0.0])), 512, 512)
        differ += int(not np.array_equal(f64_angle, want))
    assert differ > 0          # the float64-angle form is a different raster on some of them: the test has teeth


def test_affine_source_index_equals_grid_sample(golden_dir):
    """The source index of every output pixel (an index image makes grid_sample return it), for matrices with rotation
    AND fractional translation, non-square and non-power-of-two sizes: pins the operation order of the float32 grid
    (k-ordered FMA chain of the sgemm) and of the unnormalisation."""
    g17 = _load(golden_dir, "g17_torch_resample.npz")
    for key, h, w, m in _affine_cases():
        idx = np.arange(1, h * w + 1, dtype=np.float32).reshape(h, w)
        want = _recorded(g17, key, _f64_grid_sample(idx, m)).astype(np.int64) - 1          # -1: zero fill
        ii, jj = E.affine_source_index(h, w, m)
        ok = (ii >= 0) & (ii < h) & (jj >= 0) & (jj < w)
        got = np.where(ok, ii * w + jj, -1)
        assert np.array_equal(got, want)


def test_disc_raster_rule():
    occ = E.disc_raster([[4.5, 2.5, 1.0]], 8)               # [col, row, r]: centre of pixel (2,4)
    assert occ[2, 4] and occ[1, 4] and occ[3, 4] and occ[2, 3] and occ[2, 5]
    assert occ.sum() == 5
    assert E.disc_raster(np.zeros([0, 3]), 8).sum() == 0


# ------------------------------------------------------------------ G14 label masks (next row)
def test_mask_path_matches_reference(golden_dir):
    g = _load(golden_dir, "g14_gen_path.npz")
    prec = dict(space=np.zeros([224, 224], bool))
    for pts, want in zip(g["pathpoint"], g["mask"]):
        mp, _ = E.label_masks(prec, 0.0, [0, 0], pts, 224, bound=224)
        assert np.array_equal(mp, want)


# ------------------------------------------------------------------ G15: how far the disc rule is from the reference's raster
def test_disc_raster_deviation_from_reference_plot_obstacles(golden_dir, capsys):
    """A13 is modelled, not reproduced bit for bit: Path.plot_obstacles (Path.py:36-49) goes matplotlib (1 pt black stroke,
    antialiased) -> JPEG -> PIL '1' (Floyd-Steinberg dither) -> crop -> Resize, and is not integer-reproducible.  g15 holds the
    reference's own function run in the build container (stand-ins: ToTensor, Resize = bilinear without antialiasing) on 21
    config-1 obstacle lists; this test MEASURES the build's rule against it.  The rule models the geometry of that pipeline
    (oracle/edage_np.py raster_geometry): the crop [53:383, 73:517] sits slightly inside matplotlib's axes box, so an output
    pixel shows a data point displaced by up to ~1 % of R from its own centre, and the stroke inks 0.625 figure px beyond the
    radius.  Measured: IoU 0.984-0.987 at R = 64 / 224 / 256 (0.94-0.97 for the plain "pixel centre in the disc" rule of rounds
    1-2), 0.3 % of all pixels differ, of BOTH signs (no systematic bias left), every differing pixel within 2 px of a rim."""
    g = _load(golden_dir, "g15_plot_obstacles.npz")
    rows = []
    for c in range(int(g["ncase"][0])):
        R, obs = int(g[f"c{c}_R"][0]), g[f"c{c}_obs"]
        ref = np.unpackbits(g[f"c{c}_occ"])[:R * R].reshape(R, R).astype(bool)
        mine = E.disc_raster(obs, R)
        diff = ref ^ mine
        yy, xx = np.nonzero(diff)
        rim = np.full(len(yy), np.inf)
        for cx, cy, r in obs:
            rim = np.minimum(rim, np.abs(np.sqrt((xx + 0.5 - cx) ** 2 + (yy + 0.5 - cy) ** 2) - r))
        rows.append((R, (ref & mine).sum() / (ref | mine).sum(), diff.mean(), rim.max() if len(rim) else 0.0, ref.sum() - mine.sum()))
        # the plain rule of rounds 1-2, for the record: always the smaller discs
        plain = np.zeros([R, R], bool)
        for cx, cy, r in obs:
            plain |= ((np.arange(R) + 0.5)[None, :] - cx) ** 2 + ((np.arange(R) + 0.5)[:, None] - cy) ** 2 <= r * r
        assert (ref & mine).sum() / (ref | mine).sum() > (ref & plain).sum() / (ref | plain).sum()
    iou = np.array([r[1] for r in rows])
    with capsys.disabled():
        for R in (64, 224, 256):
            sel = [r for r in rows if r[0] == R]
            print(f"\n[A13 deviation] R={R}: IoU {min(r[1] for r in sel):.3f}-{max(r[1] for r in sel):.3f}, differing pixels "
                  f"{100 * max(r[2] for r in sel):.2f} % max, farthest from a rim {max(r[3] for r in sel):.2f} px", end="")
    assert iou.min() >= 0.98 and max(r[2] for r in rows) < 0.005
    assert max(r[3] for r in rows) < 2.0                                       # rim-local: never a missing or extra disc
    # no systematic bias: over the cases of each resolution the differing pixels are of both signs
    for R in (64, 224, 256):
        more = less = 0
        for c in range(int(g["ncase"][0])):
            if int(g[f"c{c}_R"][0]) != R:
                continue
            ref = np.unpackbits(g[f"c{c}_occ"])[:R * R].reshape(R, R).astype(bool)
            mine = E.disc_raster(g[f"c{c}_obs"], R)
            more += int((ref & ~mine).sum()); less += int((mine & ~ref).sum())
        assert more > 0 and less > 0 and max(more, less) < 4 * min(more, less), (R, more, less)
