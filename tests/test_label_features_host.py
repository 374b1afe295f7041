"""makefeature.pl's stage on the CPU: the Python restatement (tests/label_features_reference.py) against the fixture the
reference's own script wrote (tools/gen_golden_ffi.py), recipe.parse_question_config / parse_label with every `die` of
the script, both engines of the library's pattern layer through WorldMi355LabelPatternMatch, its refusals, and the
float32 argument of DESIGN.md as a sweep."""
import math
import os

import numpy as np
import pytest

import label_features_reference as R
from conftest import GOLDEN

SPECIALS = "ab12-+^_@=/:|$[].x"


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "label_features.npz"))


def block(fx, name):
    n = int(fx[name + "/n_labels"])
    return (str(fx[name + "/config"]), [str(fx["%s/label%d" % (name, i)]) for i in range(n)], int(fx[name + "/frame_shift"]),
            [fx["%s/out%d" % (name, i)] for i in range(n)], [tuple(int(v) for v in fx["%s/warn%d" % (name, i)]) for i in range(n)])


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


def test_fixture_holds_what_the_stage_can_get_wrong(fx):
    config, labels, shift, outs, warns = block(fx, "random")
    verdicts = outs[0][:, :320]
    assert outs[0].shape == (200, 360) and ((verdicts == 0) | (verdicts == 1)).all()
    assert 0.2 <= (verdicts == 1).mean() <= 0.8                          # a fifth of each at least
    config, labels, shift, outs, warns = block(fx, "recipe")
    feats = R.parse_config(config)
    kinds = [k for _, k, _, _, _ in feats]
    assert len(feats) == 42 and kinds.count("float") == 11 and kinds.count("reserved") == 6
    levels = [R.parse_label(t, shift)[1] for t in labels]
    assert levels == ["state"] * 3 + ["phoneme"] * 3
    assert any(s for _, _, _, s in R.parse_label(labels[5], shift)[0])     # state-level lines in a phoneme-level file
    assert all(any(e - s == 1 for s, e, _, _ in R.parse_label(t, shift)[0]) for t in labels[:3])   # lines of one frame
    allrows = np.concatenate(outs)
    for k, (name, kind, patt, lo, hi) in enumerate(feats):
        col = allrows[:, k]
        if name == "E-never" or name in ("only-empty", "no-star"):
            assert (col == 0).all(), name
        else:
            assert len(np.unique(col)) >= 2, name                           # every other feature takes two values at least
    assert all(w[0] > 0 for w in warns) and [w[1] > 0 for w in warns] == [False] * 3 + [True] * 3


@pytest.mark.parametrize("name", ["recipe", "random"])
def test_restatement_reproduces_the_scripts_output(fx, name):
    config, labels, shift, outs, warns = block(fx, name)
    for text, want, warn in zip(labels, outs, warns):
        rows, mine = R.rows(config, text, shift)
        assert same_bits(rows, want) and tuple(mine) == warn


@pytest.mark.parametrize("name", ["recipe", "random"])
def test_recipe_parsers_on_the_fixture(fx, pkg, name):
    config, labels, shift, outs, warns = block(fx, name)
    names, features = pkg.recipe.parse_question_config(config)
    want = R.parse_config(config)
    assert names == [w[0] for w in want]
    for (kind, patt, lo, hi), (_, wkind, wpatt, wlo, whi) in zip(features, want):
        if wkind == "reserved":
            assert kind == 2 + R.RESERVED.index(_) and patt is None and (lo, hi) == (wlo, whi)
        elif wkind == "float":
            assert (kind, patt, lo, hi) == (1, wpatt, wlo, whi)
        else:
            assert (kind, patt, lo, hi) == (0, wpatt, 0, 0)
    for text, rows in zip(labels, outs):
        lines, level = pkg.recipe.parse_label(text, shift)
        wlines, wlevel = R.parse_label(text, shift)
        assert lines == wlines and level == (wlevel == "state")
        assert sum(e - s for s, e, _, _ in lines) == rows.shape[0]


def test_recipe_parsers_die_where_the_script_dies(pkg, tmp_path):
    cfg, lab = pkg.recipe.parse_question_config, pkg.recipe.parse_label
    for text, message in (("lonely\n", "Cannot specify feature type"),
                          ("a *-k+*\n", "There is not feature patten"),
                          ("a {*-k+*\n", "There is not feature patten"),
                          ("a {}\n", "There is not feature patten"),
                          ("a {*%d*%d} MIN=0 MAX=1\n", "There are multiple '%d'"),
                          ("a {*%d,*} MIN=0 MAX=1\n", "There are multiple patterns for float"),
                          ("a {*%d} MIN=0\n", "Min and max values are required"),
                          ("a {*%d} MAX=3\n", "Min and max values are required"),
                          ("a MIN=0 {*%d} MAX=3\n", "There is not feature patten"),
                          ("a {*%d} MIN=0 MAX=1.5\n", "Min and max values must be integer"),
                          ("Pos_C-Frame_in_State(Fw) MIN=x MAX=2\n", "Min and max values must be integer"),
                          ("Pos_C-Frame_in_State(Fw)\n", "Min and max values are required")):
        with pytest.raises(ValueError, match="ERROR: " + message.replace("'", ".")):
            cfg(text)
    names, feats = cfg("# c\n\n  a   {x,y}  \n\tb {*_%d} MAX=+7 MIN=-2 junk\nPos_C-Frame_in_Phone(Bw) MAX=9 MIN=1\n%d {d%}\n")
    assert names == ["a", "b", "Pos_C-Frame_in_Phone(Bw)", "%d"]
    assert feats == [(0, "x,y", 0, 0), (1, "*_%d", -2, 7), (7, None, 1, 9), (0, "d%", 0, 0)]
    for text, message in (("0 50000\n", "There is not model name"),
                          ("0\n", "There is not start/end time"),
                          ("0 50000 a\n\n50000 100000 b\n", "There is not start/end time"),
                          ("50000 50000 a\n", "There is error of start/end value"),
                          ("100000 50000 a\n", "There is error of start/end value"),
                          ("-100000 50000 a\n", "There is error of start/end value"),
                          ("0 1e30 a\n", "Start/end must be integer"),
                          ("0 50000 a[2]\n50000 100000 a\n", "There is phoneme-level line in state-level label"),
                          ("0 50000 a[2]\n50000 100000 a[1]\n", "There is phoneme-level line in state-level label"),
                          ("", "Unknown label level")):
        with pytest.raises(ValueError, match="ERROR: " + message):
            lab(text, 50000)
    lines, level = lab("0 50000 a\n50000 150000 b[3]\n150000 200000 [4]\n200000 250000 c[2]x\n250000 300000 d[+02]", 50000)
    assert not level                                                    # ... and the state-level lines are let in, cut
    assert lines == [(0, 1, "a", 0), (1, 3, "b", 3), (3, 4, "[4]", 0), (4, 5, "c[2]x", 0), (5, 6, "d", 2)]
    assert lab("24999 75000 a", 50000)[0] == [(0, 2, "a", 0)] and lab("25000 124999 a", 50000)[0] == [(1, 2, "a", 0)]
    assert lab("25000 125000 a x y", 50000)[0] == [(1, 3, "a", 0)]        # int(0.5 + t / shift); further fields are not read
    assert lab("abc 7e4 a", 50000)[0] == [(0, 1, "a", 0)]                 # Perl's numeric value of a string
    path = tmp_path / "q.conf"
    path.write_text("a {b}\n")
    assert pkg.recipe.read_question_config(str(path)) == (["a"], [(0, "b", 0, 0)])
    path = tmp_path / "a.lab"
    path.write_text("0 50000 a[2]\n")
    assert pkg.recipe.read_label(str(path), 50000) == ([(0, 1, "a", 2)], True)


def both_engines(W, patt, name):
    m0, _ = W.label_pattern_match(patt, name, engine=0)
    m1, _ = W.label_pattern_match(patt, name, engine=1)
    return m0, m1


@pytest.mark.parametrize("name", ["recipe", "random"])
def test_both_engines_against_the_fixture(fx, pkg, name):
    W = pkg.world
    config, labels, shift, outs, warns = block(fx, name)
    feats = R.parse_config(config)
    checked = 0
    for text, rows in zip(labels, outs):
        t = 0
        for start, end, lname, state in R.parse_label(text, shift)[0]:
            row = rows[t]
            t += end - start
            for k, (fname, kind, patt, lo, hi) in enumerate(feats):
                if kind == "binary":
                    assert both_engines(W, patt, lname) == (row[k] == 1, row[k] == 1), (patt, lname)
                elif kind == "float":
                    hit, value = W.label_pattern_match(patt, lname, is_float=True)
                    want = np.float32(0.0 if not hit or value < lo else 1.0 if value > hi else (value - lo) / (hi - lo))
                    assert want.view(np.uint32) == row[k].view(np.uint32), (patt, lname, hit, value)
                    assert (hit, value) == R.match_number(lname, patt)
                checked += 1
    assert checked > 5000


def random_pair(rng, n_tok, n_len):
    """A pattern of n_tok tokens and a name of n_len bytes that matches it where that is possible, then sometimes
    spoilt.  The numbers of `*` and `?` are held to what `re` can backtrack through in a failing match."""
    stars = min(6, max(1, int(math.log(2e4) / math.log(n_len + 1))))
    opts = n_tok if n_len <= 2 else 8
    kinds = []
    for _ in range(n_tok):
        r = rng.random()
        if kinds and kinds[-1] in "*?" and r < 0.5:
            r = rng.random() * 0.3                                      # runs of several `*` and `?` in a row
        k = "*" if r < 0.15 else "?" if r < 0.3 else "." if r < 0.4 else "c"
        if (k == "*" and kinds.count("*") >= stars) or (k == "?" and kinds.count("?") >= opts):
            k = "c"
        kinds.append(k)
    patt = "".join(k if k != "c" else SPECIALS[int(rng.integers(0, len(SPECIALS)))] for k in kinds)
    fixed = sum(1 for c in patt if c not in "*?")
    spare = n_len - fixed
    name = ""
    if spare >= 0:
        n_star = patt.count("*")
        for c in patt:
            pick = SPECIALS[int(rng.integers(0, len(SPECIALS)))]
            if c == "*":
                run = spare if n_star == 1 else int(rng.integers(0, spare + 1))
                name += "".join(SPECIALS[int(i)] for i in rng.integers(0, len(SPECIALS), run))
                spare -= run
                n_star -= 1
            elif c == "?":
                if spare > 0 and rng.random() < 0.5:
                    name += pick
                    spare -= 1
            else:
                name += pick if c == "." else c
    if len(name) != n_len:                                              # no way to fill it: a random name
        name = "".join(SPECIALS[int(i)] for i in rng.integers(0, len(SPECIALS), n_len))
    elif rng.random() < 0.4:
        at = int(rng.integers(0, n_len))
        name = name[:at] + "1" + name[at + 1:]
    return patt, name


def test_both_engines_against_the_restatement_on_random_pairs(pkg):
    W = pkg.world
    rng = np.random.default_rng(5)
    shapes = [(t, n) for t in (1, 31, 32, 33, 63) for n in (1, 63, 64, 65, 1023)] + [(t, n) for t in range(1, 13) for n in (2, 5, 17)]
    hits = total = 0
    for n_tok, n_len in shapes:
        seen = 0
        for _ in range(60):
            patt, name = random_pair(rng, n_tok, n_len)
            want = R.match(name, patt)
            assert both_engines(W, patt, name) == (want, want), (patt, name)
            seen += want
            total += 1
        hits += seen
    print("%d pairs, %d of them match" % (total, hits))
    assert total >= 3000 and 0.2 * total <= hits <= 0.8 * total
    # comma-separated alternatives: any of them
    for _ in range(300):
        alts = [random_pair(rng, int(rng.integers(1, 9)), 6)[0] for _ in range(int(rng.integers(1, 5)))]
        name = random_pair(rng, 4, 6)[1]
        want = R.binary(name, ",".join(alts))
        assert both_engines(W, ",".join(alts), name) == (want, want)
    # float patterns: the capture under Perl's backtracking order
    for _ in range(600):
        head, tail = random_pair(rng, int(rng.integers(0, 5)), 4)[0], random_pair(rng, int(rng.integers(0, 5)), 4)[0]
        name = "".join("ab_+-0123456789"[int(i)] for i in rng.integers(0, 15, int(rng.integers(1, 30))))
        patt = head + "%d" + tail
        assert W.label_pattern_match(patt, name, is_float=True) == R.match_number(name, patt), (patt, name)
    assert W.label_pattern_match("*_%d*", "a_1_22_333", True) == (True, 333)
    assert W.label_pattern_match("*_%d_*", "a_1_22_333", True) == (True, 22)
    assert W.label_pattern_match("*_%d?3", "a_1_22_333", True) == (True, 33)
    assert W.label_pattern_match("a%d", "a-007", True) == (True, -7)
    assert W.label_pattern_match("a%d", "a+-7", True) == (False, 0)
    assert W.label_pattern_match("a%d", "a99999999999999999999", True) == (True, 2 ** 31 - 1)     # saturates
    many = "*a" * 31 + "*"                                              # 63 tokens, 32 of them `*`: remembered failures
    assert both_engines(W, many, "a" * 30 + "b" * 900) == (False, False)
    assert both_engines(W, many, "ab" * 31) == (True, True)


def test_refusals(pkg):
    W = pkg.world
    refused = lambda kind: pytest.raises(RuntimeError, match=kind)
    for engine in (0, 1):
        for patt in ("a\\b", "a(b", "a)b", "a{b", "a}b", "a b", "a\tb", "a\x7fb", "a\xe9b", "*" * 64, "a" * 64):
            with refused("unsupported"):
                W.label_pattern_match(patt, "ab", engine=engine)
        for name in ("a b", "a\x7f", "\xe9", "a" * 1024):
            with refused("unsupported"):
                W.label_pattern_match("*", name, engine=engine)
        with refused("bad argument"):
            W.label_pattern_match("*", "", engine=engine)
        assert W.label_pattern_match("*", "a" * 1023, engine=engine) == (True, 0)
        assert W.label_pattern_match("?" * 63, "a" * 63, engine=engine) == (True, 0)
        assert W.label_pattern_match("a,,b", "b", engine=engine) == (True, 0)           # an empty alternative is valid
        assert W.label_pattern_match(",", "b", engine=engine) == (False, 0)             # ... and matches nothing
        assert W.label_pattern_match("", "b", engine=engine) == (False, 0)
    assert W.label_pattern_match("a%d", "a%d", engine=1) == (True, 0)                   # binary: `%` and `d` are literals
    for patt in ("a", "%d%d", "a%d,b", "a%d,b%d"):
        with refused("bad argument"):
            W.label_pattern_match(patt, "a1", is_float=True)
    with refused("bad argument"):
        W.label_pattern_match("a%d", "a1", is_float=True, engine=1)                     # engine 1 is for binary patterns
    with refused("bad argument"):
        W.label_pattern_match("a", "a", engine=2)
    with refused("unsupported"):
        W.label_pattern_match("a" * 62 + "%d" + "b", "a1", is_float=True)               # %d is one token: 64
    assert W.label_pattern_match("a" * 61 + "%d" + "b", "a" * 61 + "5b", is_float=True) == (True, 5)


def test_one_rounding_equals_the_text_round_trip():
    """for 0 <= n <= d <= 2^20, float32(n / d) -- one rounding of the double quotient -- has the bits of the
    script's path, 15 significant digits of text parsed back to a double and cast.  Every denominator up to 1500, and
    several up to 2^20 with every numerator of a stride."""
    def check(n, d):
        q = n / d
        text = np.array([float("%.15g" % v) for v in q])
        a, b = q.astype(np.float32), text.astype(np.float32)
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), d
        return len(q)
    count = 0
    for d in range(1, 1501):
        count += check(np.arange(d + 1, dtype=np.float64), float(d))
    for d in (2 ** 20, 2 ** 20 - 1, 2 ** 20 - 3, 1000003 if 1000003 <= 2 ** 20 else 1000000, 999983, 786433, 524289, 65537, 40961):
        count += check(np.arange(0, d + 1, 97, dtype=np.float64), float(d))
        count += check(np.arange(max(0, d - 2000), d + 1, dtype=np.float64), float(d))
    print("%d quotients" % count)
    assert count > 1_100_000
