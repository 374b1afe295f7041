"""The `ffo` / `stats` / GV-data stages on the CPU: tests/ffo_reference.py against the golden the reference's own Perl
scripts wrote (tools/gen_golden_ffo.py), world.pool_moments against long double, the row layout, the command line and
the argument checks that need no device."""
import os

import numpy as np
import pytest

import ffo_reference as R
from conftest import GOLDEN

U = 2.0 ** -53
LENGTHS = (1, 2, 3, 5, 63, 64, 65, 130, 257)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "recipe_ffo.npz"))


def ffo_case(fx):
    names = [str(n) for n in fx["ffo/names"]]
    streams = [(int(d), [list(fx["ffo/%s_win%d" % (n, i)]) for i in (1, 2, 3)], bool(m))
               for n, d, m in zip(names, fx["ffo/dims"], fx["ffo/msd"])]
    return [fx["ffo/" + n] for n in names], streams


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


def test_golden_holds_the_cases_the_kernel_can_get_wrong(fx):
    seen = set()
    for dim in (1, 2):
        for T in LENGTHS:
            x = fx["ip/d%d_T%d/x" % (dim, T)]
            assert x.shape == (T, dim)
            for c in range(dim):
                valid = np.nonzero(x[:, c] != np.float32(-1e10))[0]
                assert len(valid) > 0
                seen |= {"leading"} if valid[0] > 0 else set()
                seen |= {"trailing"} if valid[-1] < T - 1 else set()
                seen |= {"only first"} if T > 1 and list(valid) == [0] else set()
                seen |= {"only last"} if T > 1 and list(valid) == [T - 1] else set()
                for lo, hi in zip(valid[:-1], valid[1:]):
                    seen |= {"long"} if hi - lo - 1 > 64 else set()
                    seen |= {"across 64"} if hi - lo > 1 and (lo + 1) // 64 != (hi - 1) // 64 else set()
    assert seen == {"leading", "trailing", "only first", "only last", "long", "across 64"}
    gaps = np.concatenate([(fx["ip/d%d_T%d/x" % (d, T)] == np.float32(-1e10)).ravel() for d in (1, 2) for T in LENGTHS])
    assert 0.35 < gaps.mean() < 0.75


@pytest.mark.parametrize("dim", [1, 2])
def test_helper_interpolation_has_the_scripts_bits(fx, dim):
    for T in LENGTHS:
        key = "ip/d%d_T%d" % (dim, T)
        out, voiced, status = R.interpolate(fx[key + "/x"])
        assert status == 0 and same_bits(out, fx[key + "/out"]), key
        assert (voiced == (fx[key + "/x"][:, 0] != np.float32(-1e10))).all()


def test_helper_ffo_rows_have_the_scripts_bits(fx, pkg):
    feats, streams = ffo_case(fx)
    rows, status = R.ffo_rows(feats, streams)
    assert status == 0 and same_bits(rows, fx["ffo/rows"])
    layout, width = pkg.recipe.ffo_layout(streams)
    assert width == rows.shape[1] == 28 and layout == [(None, 0, 15), (15, 16, 3), (None, 19, 9)]
    assert (rows[:, 15] == (feats[1][:, 0] != np.float32(-1e10))).all()      # the voicing flag sits in the layout's column
    # a stream without a valid value: status 1 and zeros where the script dies
    out, voiced, status = R.interpolate(np.full((5, 1), -1e10, dtype=np.float32))
    assert status == 1 and (out == 0).all() and (voiced == 0).all()


def test_helper_other_gap_markers():
    x = np.array([[0.0], [5.0], [0.0], [0.0], [6.5], [0.0]], dtype=np.float32)
    out, voiced, status = R.interpolate(x, 0.0)
    assert status == 0 and list(out[:, 0]) == [5.0, 5.0, 5.5, 6.0, 6.5, 6.5] and list(voiced) == [0, 1, 0, 0, 1, 0]
    y = np.where(x == 0, np.float32(1e-8), x)
    assert same_bits(R.interpolate(y, 1e-8)[0], out)
    assert same_bits(R.interpolate(y, -1e10)[0], y)                        # nothing is a gap: copied


def parts_of(x, cuts):
    return [R.moments(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def as_f64(parts):
    return (np.stack([p[0] for p in parts]), np.stack([p[1].astype(np.float64) for p in parts]),
            np.stack([p[2].astype(np.float64) for p in parts]))


@pytest.mark.parametrize("seed", range(6))
def test_pool_moments_against_long_double(pkg, seed):
    """Random splits into up to 4 parts, some of them empty: the pooled variance equals the long-double variance of the
    concatenation to 8 * 2^-53 relative, also when two triples pooled earlier are pooled again."""
    rng = np.random.default_rng(seed)
    n, width = 1000, 5
    x = (rng.standard_normal((n, width)) + rng.uniform(-1, 1, width)).astype(np.float32)
    cnt, _, m2 = R.moments(x)
    want = m2 / cnt.astype(R.LD)
    inner = sorted(rng.integers(0, n + 1, 3))
    cuts = [0] + inner + [n]
    if seed % 2:
        cuts = [0, 0] + inner[:1] + inner[:1] + inner[1:2] + [n, n]        # empty parts: in front, inside, at the end
    parts = parts_of(x, cuts)
    c, m, s = as_f64(parts)
    pn, pm, ps = pkg.world.pool_moments(c, m, s)
    assert pn.dtype == np.int64 and (pn == n).all() and pm.dtype == ps.dtype == np.float64
    err = np.abs(ps.astype(R.LD) / R.LD(n) - want) / want
    print("seed %d: %d parts, worst error / bound %.3f" % (seed, len(parts), float(err.max()) / (8 * U)))
    assert (err <= 8 * U).all()
    assert (np.abs(pm.astype(R.LD) - x.astype(R.LD).mean(axis=0)) <= 8 * U * np.abs(x).mean(axis=0)).all()
    # associative: (first k parts) + (the rest), each pooled on its own first
    for k in range(len(parts) + 1):
        a = pkg.world.pool_moments(c[:k], m[:k], s[:k])
        b = pkg.world.pool_moments(c[k:], m[k:], s[k:])
        qn, qm, qs = pkg.world.pool_moments(*[np.stack(t) for t in zip(a, b)])
        assert (qn == n).all()
        assert (np.abs(qs.astype(R.LD) / R.LD(n) - want) / want <= 8 * U).all(), k


def test_pool_moments_edges(pkg):
    n, m, s = pkg.world.pool_moments(np.zeros((3, 2), np.int64), np.full((3, 2), np.nan), np.full((3, 2), np.nan))
    assert (n == 0).all() and (m == 0).all() and (s == 0).all()            # empty parts carry no value
    n, m, s = pkg.world.pool_moments(np.zeros((0, 4), np.int64), np.zeros((0, 4)), np.zeros((0, 4)))
    assert n.shape == (4,) and (n == 0).all() and (s == 0).all()
    n, m, s = pkg.world.pool_moments([[2, 0]], [[1.5, 9.0]], [[0.5, 9.0]])
    assert list(n) == [2, 0] and list(m) == [1.5, 0.0] and list(s) == [0.5, 0.0]
    with pytest.raises(ValueError):
        pkg.world.pool_moments(np.ones((2, 3), np.int64), np.zeros((2, 3)), np.zeros((3, 2)))
    with pytest.raises(ValueError):
        pkg.world.pool_moments(np.ones(3, np.int64), np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError):
        pkg.world.pool_moments([[-1]], [[0.0]], [[0.0]])


def test_helper_pooled_and_gv():
    rng = np.random.default_rng(3)
    utts = [rng.standard_normal((T, 4)).astype(np.float32) for T in (7, 30, 1)]
    n, _, m2 = R.pooled([R.moments(u) for u in utts])
    assert (n == 38).all()
    assert np.allclose((m2 / 38).astype(np.float64), R.corpus_variance(utts).astype(np.float64), rtol=1e-15)
    v = np.stack([u.astype(np.float64).var(axis=0) for u in utts])
    assert np.allclose(R.gv(utts).astype(np.float64), v.var(axis=0), rtol=1e-12)


def test_sum_of_squares_fails_where_two_passes_do_not():
    """The case tests/test_gpu_ffo.py gives the device: around 1e4 with a spread of 1e-2, sum x^2 - (sum x)^2 / T in
    double is off by about 1e-5 of m2 (the helper asserts the gap to the two-pass bound when it makes the case)."""
    x = R.large_offset_case()
    v = x[:, 0].astype(np.float64)
    rel = abs((v * v).sum() - v.sum() ** 2 / len(v) - float(R.moments(x)[2][0])) / float(R.moments(x)[2][0])
    print("sum of squares: relative error %.2e" % rel)
    assert 1e-7 < rel < 1e-3


def test_cli_parses_the_new_subcommands(pkg, tmp_path, capsys):
    scp = tmp_path / "empty.scp"
    scp.write_text("")
    w1, w2 = str(tmp_path / "x.win1"), str(tmp_path / "x.win2")
    (tmp_path / "x.win1").write_text("1 1.0\n")
    (tmp_path / "x.win2").write_text("3 -0.5 0.0 0.5\n")
    main = pkg.recipe.main
    assert main(["ffo", "--scp", str(scp), "--stream", "5:0:" + w1, "--stream", "1:1:%s,%s" % (w1, w2), "--resume"]) == 0
    assert main(["stats", "--scp", str(scp), "--stream", "5:0:" + w1, "--out-dir", str(tmp_path / "stats"),
                 "--name", "mgc"]) == 0
    assert main(["gv-data", "--scp", str(scp), "--stream", "5:0:", "--stream", "1:1:", "--sampling-rate", "48000",
                 "--frame-shift", "240", "--silence", "pau", "--resume"]) == 0
    assert capsys.readouterr().out.count("complete. 0 frames") == 2
    assert not (tmp_path / "stats").exists()                               # nothing counted, nothing written
    for argv in (["ffo", "--scp", str(scp)], ["stats", "--scp", str(scp), "--stream", "1:0:w"],
                 ["gv-data", "--scp", str(scp), "--stream", "1:0:", "--sampling-rate", "48000"]):
        with pytest.raises(SystemExit):
            main(argv)


def test_compose_cmp_refuses_bad_arguments_without_a_device(pkg):
    """WorldMi355ComposeCmp checks its arguments on the host, as ComposeFfo does, before it looks at the batch: each of
    these returns WM_ERR_BAD_ARG (2) and makes no device call."""
    import ctypes as C
    lib = pkg.load_library()
    x, out = np.zeros((3, 2), dtype=np.float32), np.zeros((3, 4), dtype=np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    data, dims = (C.c_void_p * 1)(vp(x)), (C.c_int * 1)(2)
    nwin, wptrs, sptrs, keep = pkg.world._window_tables([[[1.0], [-0.5, 0.0, 0.5]]])
    assert list(nwin) == [2] and [sptrs[0][i] for i in range(2)] == [1, 3] and wptrs[0][1][2] == 0.5
    call = lib.WorldMi355ComposeCmp
    assert call(None, 1, data, dims, nwin, wptrs, sptrs, vp(out)) == 2          # a null batch, everything else valid
    assert call(None, 1, data, None, nwin, wptrs, sptrs, vp(out)) == 2          # null dims
    assert call(None, 0, data, dims, nwin, wptrs, sptrs, vp(out)) == 2          # no streams
    assert call(None, 5, data, dims, nwin, wptrs, sptrs, vp(out)) == 2          # more streams than the kernels hold
    assert lib.WorldMi355ComposeFfo(None, 1, data, dims, nwin, wptrs, sptrs, None, vp(out)) == 2
    del keep


def test_file_checks_raise_value_error(pkg, tmp_path):
    streams = [(2, [[1.0]], False), (1, [[1.0]], True)]
    a, b, out = (str(tmp_path / n) for n in ("a.mgc", "a.lf0", "a.ffo"))
    np.zeros((6, 2), dtype=np.float32).tofile(a)
    np.zeros(5, dtype=np.float32).tofile(b)
    with pytest.raises(ValueError, match="frames"):                        # frame counts disagree
        pkg.recipe.ffo_files([(a, b, out)], streams)
    with pytest.raises(ValueError):                                        # a path is missing from the job
        pkg.recipe.ffo_files([(a, out)], streams)
    with pytest.raises(ValueError, match="frames"):
        pkg.recipe.gv_data_files([(a, b, None, out)], streams, 48000, 240)
    np.zeros(7, dtype=np.float32).tofile(a)
    with pytest.raises(ValueError):                                        # no rows of 2 float32
        pkg.recipe.ffo_files([(a, b, out)], streams)
    with pytest.raises(ValueError):                                        # no rows of the layout's 4 float32
        pkg.recipe.stats_files([a], streams, str(tmp_path / "stats"))
    with pytest.raises(ValueError):                                        # fewer names than streams
        pkg.recipe.stats_files([], streams, str(tmp_path / "stats"), names=("mgc",))
    assert not os.path.exists(out)
