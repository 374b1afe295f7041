"""Writes tests/golden/label_features.npz: the acoustic model's input rows, produced by RUNNING the reference's own
data/scripts/makefeature.pl on hand-made question configs and label files (the reference ships neither).  Inputs and
the script's outputs are stored; nothing of the script itself.  SPTK is not needed: `x2x +af` parses each printed value
to a double and casts it, which is numpy.float32(float(text)) here.

    WORLD_REFERENCE=<the reference's tree> python tools/gen_golden_ffi.py        (needs perl; no GPU)

Block `recipe`: 42 features -- every token kind, alternatives of which only the last matches, an empty alternative, `?`
matching zero and one character, `.`, the escaped characters, float features with a sign, with leading zeros, clamped
low and high, captures that depend on greediness, all six reserved features -- and six label files: three state-level,
two phoneme-level (one with `[1]` suffixes, which are no state indices) and one phoneme-level file with state-level
lines in it (the script's misspelt level check).  Several lines are one frame long.

Block `random`: 320 binary patterns of 1-12 tokens in 1-3 alternatives and 40 float patterns over the alphabet
`a b - + ^ _ @ 1 2`, against 200 one-frame lines with names of 1-40 bytes.  Asserted here and again by the tests: at
least a fifth of the binary verdicts are 1 and at least a fifth are 0.

Per block the fixture holds the config text, the label texts, the frame shift, the script's output as float32 and the
count of each warning on its stderr.  tests/label_features_reference.py is compared with every output and the number of
differing values printed.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import label_features_reference as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "label_features.npz")
FRAME_SHIFT = 50000

RECIPE_CONFIG = """# a question config in makefeature.pl's format
C-sil            {*-sil+*}
C-pau            {*-pau+*}
C-vowel          {*-a+*,*-i+*,*-u+*,*-e+*,*-o+*}
C-nasal          {*-n+*,*-N+*}
C-one-char       {*-?+*}
C-k-or-kx        {*-k?+*}
C-c-then-one     {*-c?+*}
C-two-opt        {*-??+*}
   L-sil         {*^sil-*}
R-sil            {*+sil=*}
LL-x             {x^*}
LL-any-one       {.^*}
ends-3           {*$f/E:*3}
bar-x            {*|x$*}
plus-o           {*+o=*}
C-dot-b          {*/C:a.b/*}
C-opt-b          {*/C:a.?b/*}
C-star-star      {*/C:**.b/*}
empty-alt        {*-zz+*,,*-k+*}
only-empty       {,}
bracket-1        {*[1]}
bracket-any      {*[?]}
whole-name       {x^sil-k+o=N/*}
no-star          {sil}
at-pos           {*@1/*,*@2/*}
A1               {*/A:%d+*}      MIN=-5 MAX=5
A2               {*+%d_*}        MIN=0 MAX=4
A3-leading-zero  {*_%d/B:*}      MIN=0 MAX=20
D-clamped        {*/D:%d|*}      MIN=-10 MAX=10
D-after-plus     {*/D:+%d|*}     MIN=0 MAX=32
E-last           {*_%d*}         MIN=0 MAX=400
E-middle         {*_%d_*}        MIN=0 MAX=400
E-first          {*:_%d*}        MIN=0 MAX=400
E-opt            {*_%d?}         MAX=400 MIN=0
E-opt-3          {*_%d?3}        MIN=0 MAX=400
E-never          {*/Z:%d*}       MIN=0 MAX=1
Pos_C-State_in_Phone(Fw)   MIN=2 MAX=6
Pos_C-State_in_Phone(Bw)   MIN=2 MAX=6
Pos_C-Frame_in_State(Fw)   MIN=1 MAX=5
Pos_C-Frame_in_State(Bw)   MIN=1 MAX=5
Pos_C-Frame_in_Phone(Fw)   MIN=1 MAX=20
Pos_C-Frame_in_Phone(Bw)   MIN=2 MAX=20
"""

PHONES = ("sil", "k", "o", "N", "n", "i", "ch", "i", "w", "a", "kx", "e", "pau", "u", "sil")


def names(rng, phones):
    ctx = ("x", "x") + tuple(phones) + ("x", "x")
    out = []
    for i, p in enumerate(phones):
        a1, a2, a3 = int(rng.integers(-7, 8)), int(rng.integers(0, 7)), int(rng.integers(0, 25))
        d = int(rng.integers(-20, 21))
        c = ("a.b", "axb", "ab", "axyb", "a..b", "b")[int(rng.integers(0, 6))]
        e = "_%d_%d_%d" % (int(rng.integers(0, 10)), int(rng.integers(10, 100)), (333, 13, 3, 450)[int(rng.integers(0, 4))])
        out.append("%s^%s-%s+%s=%s/A:%d+%d_%02d/B:%d@%d/C:%s/D:%+d|%s$f/E:%s" % (
            ctx[i], ctx[i + 1], p, ctx[i + 3], ctx[i + 4], a1, a2, a3, i + 1, len(phones) - i, c, d, "xy"[int(rng.integers(0, 2))], e))
    return out


def label_text(rng, lines, jitter=True):
    """lines: [(frames, name)] one after another, the boundaries off the frame grid by less than half a frame."""
    text, t = "", 0
    for frames, name in lines:
        a = t * FRAME_SHIFT + (int(rng.integers(-20000, 20001)) if jitter and t > 0 else 0)
        t += frames
        b = t * FRAME_SHIFT + (int(rng.integers(-20000, 20001)) if jitter else 0)
        text += "%d %d %s\n" % (a, b, name)
    return text


def recipe_labels():
    rng = np.random.default_rng(20)
    labels = []
    for f in range(3):                                               # state-level: five states per phoneme
        lines = []
        for name in names(rng, PHONES[f:f + 9]):
            for s in range(2, 7):
                lines.append((int(rng.choice([1, 1, 2, 3, 5, 8])), "%s[%d]" % (name, s)))
        labels.append(label_text(rng, lines))
    lines = [(int(rng.integers(1, 30)), name) for name in names(rng, PHONES[5:15])]
    labels.append(label_text(rng, lines))                            # phoneme-level
    lines = [(int(rng.integers(1, 12)), name + "[1]") for name in names(rng, PHONES[:8])]
    labels.append("  " + label_text(rng, lines, jitter=False).replace(" ", "\t "))   # ... `[1]` is no state index
    lines = [(int(rng.integers(1, 9)), name + ("[%d]" % (2 + i % 3) if i else "")) for i, name in
             enumerate(names(rng, PHONES[4:13]))]
    labels.append(label_text(rng, lines))                            # phoneme-level by its first line, state-level lines after it
    return labels


ALPHABET = "ab-+^_@12"


def random_pattern(rng, lo, hi):
    n = int(rng.integers(lo, hi + 1))
    out = ""
    for k in rng.random(n):
        pick = ALPHABET[int(rng.integers(0, len(ALPHABET)))]
        if k < 0.42 and out.count("*") >= 3:                          # a failing match costs length^stars in a backtracking
            k = 0.5 + 0.5 * k                                         # matcher without memory, such as the test suite's witness
        out += "*" if k < 0.42 else "?" if k < 0.52 else "." if k < 0.57 else pick
    return out


def random_block():
    rng = np.random.default_rng(21)
    config = ""
    for k in range(320):
        alts = [random_pattern(rng, 1, 12) for _ in range(int(rng.integers(1, 4)))]
        config += "B%d {%s}\n" % (k, ",".join(alts))
    for k in range(40):
        lo = int(rng.integers(-3, 4))
        config += "F%d {%s%%d%s} MIN=%d MAX=%d\n" % (k, random_pattern(rng, 0, 5), random_pattern(rng, 0, 5), lo,
                                                     lo + int(rng.integers(1, 40)))
    label, t = "", 0
    for _ in range(200):
        name = "".join(ALPHABET[int(i)] for i in rng.integers(0, len(ALPHABET), int(rng.integers(1, 41))))
        label += "%d %d %s\n" % (t * FRAME_SHIFT, (t + 1) * FRAME_SHIFT, name)
        t += 1
    return config, [label]


def run_script(script, config, label):
    with tempfile.TemporaryDirectory() as tmp:
        cpath, lpath = os.path.join(tmp, "q.conf"), os.path.join(tmp, "a.lab")
        with open(cpath, "w") as f:
            f.write(config)
        with open(lpath, "w") as f:
            f.write(label)
        n = int(subprocess.run(["perl", script, cpath], capture_output=True, check=True, text=True).stdout)
        r = subprocess.run(["perl", script, cpath, str(FRAME_SHIFT), lpath], capture_output=True, check=True, text=True)
    values = np.array([np.float32(float(v)) for v in r.stdout.split()], dtype=np.float32)
    warn = (sum(1 for ln in r.stderr.splitlines() if ln.startswith("WARNING: Out of range")),
            sum(1 for ln in r.stderr.splitlines() if ln.startswith("WARNING: There is not state-level")))
    assert warn[0] + warn[1] == len(r.stderr.splitlines()), r.stderr[:400]
    return values.reshape(-1, n), warn


def main():
    ref = os.environ.get("WORLD_REFERENCE")
    if not ref:
        raise SystemExit("set WORLD_REFERENCE to the reference's tree")
    script = os.path.join(ref, "data", "scripts", "makefeature.pl")
    out, differ = {}, 0
    for block, (config, labels) in (("recipe", (RECIPE_CONFIG, recipe_labels())), ("random", random_block())):
        out[block + "/config"] = np.array(config)
        out[block + "/frame_shift"] = np.int64(FRAME_SHIFT)
        out[block + "/n_labels"] = np.int64(len(labels))
        for i, label in enumerate(labels):
            rows, warn = run_script(script, config, label)
            out["%s/label%d" % (block, i)] = np.array(label)
            out["%s/out%d" % (block, i)] = rows
            out["%s/warn%d" % (block, i)] = np.array(warn, dtype=np.int64)
            mine, mine_warn = R.rows(config, label, FRAME_SHIFT)
            differ += int((mine.view(np.uint32) != rows.view(np.uint32)).sum()) + int(tuple(mine_warn) != tuple(warn))
            print("%s %d: rows %s, warnings %s" % (block, i, rows.shape, warn))
    verdicts = out["random/out0"][:, :320]
    ones = float((verdicts == 1).mean())
    print("random: %.3f of the binary verdicts are 1, %.3f of the float values are not 0" % (
        ones, float((out["random/out0"][:, 320:] != 0).mean())))
    assert ((verdicts == 0) | (verdicts == 1)).all() and 0.2 <= ones <= 0.8
    np.savez_compressed(OUT, **out)
    print("label_features ok: %d values or warning counts differ from the Python restatement, %d bytes" % (
        differ, os.path.getsize(OUT)))


if __name__ == "__main__":
    sys.exit(main())
