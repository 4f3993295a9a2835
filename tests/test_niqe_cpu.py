"""NIQE on the host: super_resolution_amd/niqe.py against the reference's recorded results (tests/golden/niqe.npz, written by
tests/golden/gen_golden_niqe.py from basicsr/metrics/niqe.py), the metric registry, the search for the pristine model and the
argument checks of the C entries.  No GPU.

niqe.py is written in the reference's dtypes, so it agrees to round-off:
  first scale    the normalised plane equals the reference's bit for bit; the 18 features agree to 1e-12 relative (measured
                 2e-15) on every image: even numpy's pairwise float32 sums are the same sums.
  second scale   the half-size image differs from the reference's by fp32 ulps (it sums with Tensor.mv, resize.py with k
                 ascending; resize.error_bound), which then passes through the float32 sums.  The bar for what two summation
                 orders of the same float32 data do is measured here: the host definition with its block sums added in
                 float32 (numpy's pairwise order) against the same values added in fp64 moves the score by at most 1.21e-6 and
                 a feature by at most 9.1e-6 relative over the golden images (test_bars_are_measured); score and features are
                 asked to agree with the reference within 10 x that (seen: score 2.5e-8 to 3.2e-6, features to 4.6e-5).
                 The image `smooth` is left out of the second scale's FEATURE comparison: there sigma is a float32
                 cancellation, and one ulp in the half-size image re-rolls its rounding (gen_golden_niqe.py's note: over seeds
                 the host lands 2e-6 to 1e-2 from the reference; the recorded seed is one where both orders lead to the same
                 score, 1.8e-6 apart).  Its first scale and its score are compared like every other image's.
"""
import ctypes as C
import os

import numpy as np
import pytest

from niqe_cases import COUNT_COLUMNS, MEASURED_SCORE, MEASURED_SUM, SCORE_BAR, SUM_BAR, SUM_COLUMNS, checkerboard_frame, golden
from super_resolution_amd import metrics as M
from super_resolution_amd import niqe

FEATURE_BAR = 10 * 9.1e-6   # relative, against max(|feature|, 1e-3)


@pytest.fixture(scope="module")
def g():
    return golden()


@pytest.fixture(scope="module")
def host(g):
    """Per golden image: the plane, the float32-sum and fp64-sum stats, features and scores; computed once."""
    out = {}
    pris = niqe.pris_params(g["pris"])
    for c in g["cases"]:
        name = c["name"]
        plane = niqe.y_plane(g[name + "_img"], c["crop_border"])
        r = {"plane": plane}
        for tag, acc in (("32", np.float32), ("64", np.float64)):
            s1, s2 = niqe.stats_of(plane, acc)
            f = np.concatenate([niqe.features_from_stats(s1, 96), niqe.features_from_stats(s2, 48)], axis=1)
            r["stats" + tag], r["feat" + tag], r["score" + tag] = (s1, s2), f, niqe.score(f[:, :18], f[:, 18:], pris)
        out[name] = r
    return out


def _rel(a, b, floor):
    with np.errstate(all="ignore"):
        return np.abs(a - b) / np.maximum(np.abs(b), floor)


def test_window_is_the_files(g):
    w = niqe.gaussian_window()
    assert w.shape == (7, 7) and w.dtype == np.float64 and np.array_equal(w, w[::-1, ::-1]) and np.array_equal(w, w.T)
    assert np.abs(w - g["gaussian_window"]).max() <= 2e-17


def test_mscn_plane_is_the_references(g, host):
    n = niqe.mscn(host["strip"]["plane"])
    assert n.dtype == np.float32 and np.array_equal(n, g["strip_mscn"])


def test_features_and_score_against_the_reference(g, host):
    for c in g["cases"]:
        name = c["name"]
        want, got = g[name + "_feat"], host[name]["feat32"]
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = ~np.isnan(want)
        r = np.where(ok, _rel(got, want, 1e-3), 0.0)
        ds = abs(host[name]["score32"] - float(g[name + "_score"]))
        print(f"NIQE-HOST {name}: feature rel scale1 {r[:, :18].max():.3e} scale2 {r[:, 18:].max():.3e}  score {host[name]['score32']!r} "
              f"reference {float(g[name + '_score'])!r} |d| {ds:.3e}")
        assert r[:, :18].max() <= 1e-12, name
        if name != "smooth":
            assert r[:, 18:].max() <= FEATURE_BAR, name
        if np.isnan(g[name + "_score"]):
            assert np.isnan(host[name]["score32"]), name
        else:
            assert ds <= SCORE_BAR, name


def test_bars_are_measured(g, host):
    """MEASURED_SCORE / MEASURED_SUM (niqe_cases.py) are what float32 and fp64 block sums differ by, and not less."""
    ds, dsum, dfeat = 0.0, 0.0, 0.0
    for c in g["cases"]:
        r = host[c["name"]]
        if not np.isnan(r["score32"]):
            ds = max(ds, abs(r["score32"] - r["score64"]))
        for a, b in zip(r["stats32"], r["stats64"]):
            assert np.array_equal(a[..., COUNT_COLUMNS], b[..., COUNT_COLUMNS])
            dsum = max(dsum, float(_rel(a[..., SUM_COLUMNS], b[..., SUM_COLUMNS], 1e-300).max()))
        ok = ~np.isnan(r["feat32"])
        dfeat = max(dfeat, float(np.where(ok, _rel(r["feat64"], r["feat32"], 1e-3), 0.0).max()))
    print(f"NIQE-BARS measured: score {ds:.3e} sums {dsum:.3e} features {dfeat:.3e}")
    assert ds <= MEASURED_SCORE and dsum <= MEASURED_SUM and dfeat <= 9.1e-6
    assert ds >= 0.5 * MEASURED_SCORE and dsum >= 0.5 * MEASURED_SUM     # the constants are not padded


def test_smooth_image_tells_the_routes_apart(g, host):
    """On the smooth image an fp64 evaluation of sigma lands far outside the bar: a device that did not follow the reference's
    float32 roundings could not pass the GPU test's comparison with the reference's score."""
    s32, s64 = float(g["smooth_score"]), float(g["smooth_score64"])
    print(f"NIQE-ROUTES smooth: float32 route {s32!r} float64 route {s64!r} |d| {abs(s32 - s64):.3e}  bar {SCORE_BAR:.3e}")
    assert abs(s32 - s64) > 100 * SCORE_BAR
    assert abs(host["smooth"]["score32"] - s32) <= SCORE_BAR and abs(host["smooth"]["score64"] - s32) <= SCORE_BAR


def test_nan_cases(g, host):
    fb = host["flatblock"]["feat32"]
    rows = np.isnan(fb).any(axis=1)
    assert rows.sum() == 1 and np.isfinite(host["flatblock"]["score32"])
    bad = fb[rows][0]
    assert bad[0] == pytest.approx(0.2) and np.isnan(bad[1])      # the reference's argmin over NaNs: position 0, alpha 0.2
    flat = host["flat"]["feat32"]
    assert np.isnan(flat).any(axis=1).all() and np.isnan(host["flat"]["score32"])
    s = host["flat"]["stats64"][0]
    assert np.all(s == 0)                                            # no negative, no positive value: every sum is 0


def test_features_from_stats_equals_direct_fit(host):
    """The five sums are all an AGGD fit needs: the fit written directly on the block's maps gives the same features."""
    import math
    plane = host["mix"]["plane"]
    n = niqe.mscn(plane)
    got = niqe.features_from_stats(niqe.block_stats(n, 96), 96)
    gam, r_gam = niqe._aggd_grid()

    def fit(v):
        v = v.flatten()
        left = np.sqrt(np.float32(np.sum(v[v < 0] ** 2, dtype=np.float32) / np.float32((v < 0).sum())))
        right = np.sqrt(np.float32(np.sum(v[v > 0] ** 2, dtype=np.float32) / np.float32((v > 0).sum())))
        gh = left / right
        sq = np.sum(v[v < 0] ** 2, dtype=np.float32) + np.sum(v[v > 0] ** 2, dtype=np.float32)
        rhat = np.square(np.sum(np.abs(v), dtype=np.float32) / np.float32(v.size)) / (sq / np.float32(v.size))
        rn = (rhat * (np.power(gh, 3) + np.float32(1)) * (gh + np.float32(1))) / np.square(np.square(gh) + np.float32(1))
        a = gam[np.argmin((r_gam - np.float64(rn)) ** 2)]
        k = math.sqrt(math.gamma(1 / a) / math.gamma(3 / a))
        return a, float(left) * k, float(right) * k
    rows = []
    for j in range(3):
        for i in range(2):
            maps = niqe.block_maps(n[96 * i:96 * i + 96, 96 * j:96 * j + 96])
            a, bl, br = fit(maps[0])
            f = [a, (bl + br) / 2]
            for m in maps[1:]:
                a, bl, br = fit(m)
                f += [a, (br - bl) * (math.gamma(2 / a) / math.gamma(1 / a)), bl, br]
            rows.append(f)
    assert np.allclose(got, np.array(rows), rtol=1e-13, atol=0)


def test_checkerboard_frame_has_a_finite_score(g):
    v = niqe.calculate_niqe(checkerboard_frame(), 0, pris_params=g["pris"])
    assert np.isfinite(v)


def test_calculate_metric_niqe(g, tmp_path, monkeypatch):
    """`type: calculate_niqe` through the registry: no data['img2'] is needed, and the value is the reference's."""
    assert "calculate_niqe" in M.METRICS
    img, want = g["crop_img"], float(g["crop_score"])
    path = tmp_path / "pris.npz"
    np.savez(path, mu_pris_param=g["mu_pris_param"], cov_pris_param=g["cov_pris_param"])
    got = M.calculate_metric({"img": img}, {"type": "calculate_niqe", "crop_border": 4, "pris_params": str(path)})
    assert abs(got - want) <= SCORE_BAR
    assert M.calculate_metric({"img": img}, {"type": "calculate_niqe", "crop_border": 4, "pris_params": g["pris"]}) == got
    chw = np.ascontiguousarray(img.transpose(2, 0, 1))
    assert niqe.calculate_niqe(chw, 4, input_order="CHW", pris_params=g["pris"]) == got
    assert niqe.calculate_niqe(img[:, :, ::-1], 4, pris_params=g["pris"], bgr=True) == got
    plane = M.to_y_channel(img.astype(np.float32))[..., 0]
    assert niqe.calculate_niqe(plane, 4, input_order="HW", pris_params=g["pris"]) == got
    with pytest.raises(NotImplementedError, match="gray"):
        niqe.calculate_niqe(img, 4, convert_to="gray", pris_params=g["pris"])
    with pytest.raises(ValueError, match="at least one 96x96 block"):
        niqe.calculate_niqe(img[:99, :99], 4, pris_params=g["pris"])


def test_pristine_model_search_order(g, tmp_path, monkeypatch):
    good = tmp_path / "good.npz"
    np.savez(good, mu_pris_param=g["mu_pris_param"], cov_pris_param=g["cov_pris_param"])
    other = tmp_path / "other.npz"
    np.savez(other, mu_pris_param=g["mu_pris_param"] + 1.0, cov_pris_param=g["cov_pris_param"])
    monkeypatch.delenv(niqe.ENV_PRIS, raising=False)
    monkeypatch.setattr(niqe.importlib.util, "find_spec", lambda name: None)
    with pytest.raises(RuntimeError, match="pristine model.*pris_params.*HAT_NIQE_PRIS_PARAMS"):
        niqe.pris_params(None)
    # 3: beside an installed basicsr.metrics, found without importing anything
    pkg = tmp_path / "site" / "basicsr"
    (pkg / "metrics").mkdir(parents=True)
    np.savez(pkg / "metrics" / "niqe_pris_params.npz", mu_pris_param=g["mu_pris_param"] + 2.0, cov_pris_param=g["cov_pris_param"])

    class Spec:
        submodule_search_locations = [str(pkg)]
    monkeypatch.setattr(niqe.importlib.util, "find_spec", lambda name: Spec() if name == "basicsr" else None)
    mu = g["mu_pris_param"].reshape(-1)   # the file keeps it as (1, 36)
    assert np.array_equal(niqe.pris_params(None)[0], mu + 2.0)
    # 2: the environment variable comes before it
    monkeypatch.setenv(niqe.ENV_PRIS, str(other))
    assert np.array_equal(niqe.pris_params(None)[0], mu + 1.0)
    # 1: the argument comes first
    assert np.array_equal(niqe.pris_params(str(good))[0], mu)
    assert np.array_equal(niqe.pris_params(g["pris"])[1], g["cov_pris_param"])
    with pytest.raises(RuntimeError, match="does not exist"):
        niqe.pris_params(str(tmp_path / "missing.npz"))
    with pytest.raises(RuntimeError, match="mu_pris_param"):
        niqe.pris_params({"mu": 1})
    # the product never reads tests/golden
    src = open(niqe.__file__).read()
    assert "golden" not in src


def test_c_entries_reject_bad_arguments_without_gpu():
    """The new entries check their arguments before they touch the device: HAT_EINVAL (-1) here, where there is none."""
    from super_resolution_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    lib = _lib.load()
    H, W, n = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    q = lambda B, h, w, crop: lib.hat_niqe_workspace_bytes(B, h, w, crop, C.byref(H), C.byref(W), C.byref(n))   # noqa: E731
    assert q(2, 203, 301, 4) == 0 and (H.value, W.value) == (192, 288) and n.value == 2 * 4 * (192 * 288 * 2 + 96 * 288 + 96 * 144)
    assert q(1, 96, 96, 0) == 0 and (H.value, W.value) == (96, 96)
    assert q(1, 95, 300, 0) == -1 and q(1, 300, 103, 4) == -1 and q(0, 200, 200, 0) == -1 and q(1, 200, 200, -1) == -1
    assert lib.hat_niqe_workspace_bytes(1, 200, 200, 0, None, C.byref(W), C.byref(n)) == -1
    p = 4096   # never dereferenced: every call below fails its checks first
    assert lib.hat_niqe_y_u8(None, 900, 0, 1, 200, 300, 0, 0, p, None, None) == -1
    assert lib.hat_niqe_y_u8(p, 900, 0, 1, 200, 300, 0, 0, None, None, None) == -1
    assert lib.hat_niqe_y_u8(p, 899, 0, 1, 200, 300, 0, 0, p, None, None) == -1          # pitch below 3 w
    assert lib.hat_niqe_y_u8(p, 900, 900 * 199, 2, 200, 300, 0, 0, p, None, None) == -1  # overlapping samples
    assert lib.hat_niqe_y_u8(p, 900, 0, 1, 200, 300, 53, 0, p, None, None) == -1         # 94 rows are left
    win = (C.c_double * 49)()
    assert lib.hat_niqe_block_stats(p, 1, 192, 288, 64, win, p, None) == -1               # unknown block size
    assert lib.hat_niqe_block_stats(p, 1, 192, 290, 96, win, p, None) == -1
    assert lib.hat_niqe_block_stats(p, 1, 48, 96, 96, win, p, None) == -1
    assert lib.hat_niqe_block_stats(None, 1, 192, 288, 96, win, p, None) == -1
    assert lib.hat_niqe_block_stats(p, 1, 192, 288, 96, None, p, None) == -1
    assert lib.hat_niqe_block_stats(p, 1, 192, 288, 96, win, None, None) == -1
    assert lib.hat_imresize_plane_rows(None, p, 1, 96, 96, 48, p, p, 10, 480, None) == -1
    assert lib.hat_imresize_plane_rows(p, p, 1, 96, 96, 48, p, p, 10, 479, None) == -1   # table length
    assert lib.hat_imresize_plane_cols(p, 1, 48, 96, 48, p, p, 10, 480, 255.0, None, None) == -1
    assert lib.hat_imresize_plane_cols(p, 1, 48, 96, 48, p, p, 10, 481, 255.0, p, None) == -1
