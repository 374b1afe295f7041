"""The host-only pattern layer (csrc/labelpat.hpp, csrc/labelpat.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer,
as a stand-alone program: tests/hostsan/labelpat_harness.cpp compiles, matches and refuses over the fixture's patterns
(with the verdicts of tests/label_features_reference.py) and over malformed ones."""
import os
import subprocess

import numpy as np
import pytest

import label_features_reference as R
from conftest import GOLDEN, ROOT


def _runtime(name):
    p = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def test_pattern_layer_under_asan_ubsan(tmp_path):
    if not _runtime("libasan.so") or not _runtime("libubsan.so"):
        pytest.skip("gcc sanitizer runtimes not installed")
    fx = np.load(os.path.join(GOLDEN, "label_features.npz"))
    cases = []
    for block, every in (("recipe", 1), ("random", 7)):
        feats = R.parse_config(str(fx[block + "/config"]))
        names = []
        for i in range(int(fx[block + "/n_labels"])):
            names += [n for _, _, n, _ in R.parse_label(str(fx["%s/label%d" % (block, i)]), int(fx[block + "/frame_shift"]))[0]]
        names = sorted(set(names))[::every]
        for _, kind, patt, lo, hi in feats:
            for name in names:
                if kind == "binary":
                    cases.append((patt, name, 0, int(R.binary(name, patt)), 0))
                elif kind == "float":
                    hit, value = R.match_number(name, patt)
                    cases.append((patt, name, 1, int(hit), value))
    path = tmp_path / "cases.txt"
    path.write_text("".join("%s\t%s\t%d\t%d\t%d\n" % c for c in cases))
    exe = tmp_path / "labelpat_harness"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "hts-train-world_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsan", "labelpat_harness.cpp"),
                           os.path.join(ROOT, "hts-train-world_amd", "csrc", "labelpat.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1:halt_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0 and "labelpat ok: %d cases" % len(cases) in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
