"""data/scripts/makefeature.pl restated in plain Python: the script's own substitutions turn a pattern into a regular
expression, and `re` matches it (Python's backtracking order is Perl's for what is left: literals, `.`, `.*`, `.?`, one
group of `[+-]?[0-9]+`).  A second witness beside tests/golden/label_features.npz, which the script itself wrote
(tools/gen_golden_ffi.py): tests/test_label_features_host.py pins this file to the fixture bit for bit, then uses it on
inputs the fixture does not hold.  Nothing here is used by the library."""
import functools
import re

import numpy as np

RESERVED = ("Pos_C-State_in_Phone(Fw)", "Pos_C-State_in_Phone(Bw)", "Pos_C-Frame_in_State(Fw)",
            "Pos_C-Frame_in_State(Bw)", "Pos_C-Frame_in_Phone(Fw)", "Pos_C-Frame_in_Phone(Bw)")
INTEGER = re.compile(r"^[+-]?[0-9]+$")


@functools.lru_cache(maxsize=None)
def to_regex(patt, number=False):
    """makefeature.pl:459-466 (and :488 for a float pattern)."""
    for a, b in (("*", ".*"), ("?", ".?"), ("+", "\\+"), ("|", "\\|"), ("^", "\\^"), ("$", "\\$"), ("[", "\\["), ("]", "\\]")):
        patt = patt.replace(a, b)
    if number:
        patt = patt.replace("%d", "([+-]?[0-9]+)")
    return re.compile("^" + patt + "$")


def match(name, patt):
    return to_regex(patt).search(name) is not None


def match_number(name, patt):
    m = to_regex(patt, True).search(name)
    return (True, int(m.group(1))) if m else (False, 0)


def binary(name, patt):
    """:352-362; Perl's split drops trailing empty fields, which match no name anyway."""
    return any(match(name, p) for p in patt.split(","))


def norm(value, lo, hi):
    if value < lo:
        return False, 0.0
    if hi < value:
        return False, 1.0
    return True, (value - lo) / (hi - lo)


def parse_config(text):
    """[(name, type, pattern, min, max)]; raises ValueError where the script dies."""
    feats = []
    for line in text.split("\n"):
        line = line.strip()
        if line == "" or line.startswith("#"):
            continue
        arr = line.split()
        name, kind, patt, lo, hi = arr[0], "", "", "", ""
        if name in RESERVED:
            kind = "reserved"
        elif len(arr) > 1:
            kind = "float" if arr[1].find("%d") > 0 else "binary"
        if kind in ("float", "binary") and arr[1].find("{") == 0 and arr[1].rfind("}") == len(arr[1]) - 1:
            patt = arr[1][1:-1]
        for field in arr[{"reserved": 1, "float": 2}.get(kind, 0):]:
            if field.startswith("MIN="):
                lo = field[4:]
            elif field.startswith("MAX="):
                hi = field[4:]
        if kind == "":
            raise ValueError("Cannot specify feature type")
        if kind != "reserved" and patt == "":
            raise ValueError("There is not feature patten")
        if kind == "float" and (patt.count("%d") != 1 or "," in patt):
            raise ValueError("float pattern")
        if kind != "binary":
            if lo == "" or hi == "":
                raise ValueError("Min and max values are required")
            if not INTEGER.match(lo) or not INTEGER.match(hi):
                raise ValueError("Min and max values must be integer")
            lo, hi = int(lo), int(hi)
        feats.append((name, kind, patt, lo, hi))
    return feats


def parse_label(text, frame_shift):
    """([(start, end, name, state index)], level); raises ValueError where the script dies."""
    body = text.split("\n")
    if body and body[-1] == "":
        body.pop()
    lines, level = [], ""
    for line in body:
        arr = line.strip().split()
        if len(arr) < 2:
            raise ValueError("There is not start/end time in label")
        start, end = int(0.5 + float(arr[0]) / frame_shift), int(0.5 + float(arr[1]) / frame_shift)
        name = arr[2] if len(arr) > 2 else ""
        left, right, state = name.rfind("["), name.rfind("]"), 0
        if left > 0 and right > 0 and left < right:
            inner = name[left + 1:-1]
            if INTEGER.match(inner) and int(inner) >= 2:
                state = int(inner)
                name = name[:left]
        if end <= start or start < 0:
            raise ValueError("There is error of start/end value in label")
        if name == "":
            raise ValueError("There is not model name in label")
        if level == "":
            level = "state" if state else "phoneme"
        elif level == "state" and not state:
            raise ValueError("There is phoneme-level line in state-level label")
        lines.append((start, end, name, state))
    if level == "":
        raise ValueError("Unknown label level")
    return lines, level


def as_float32(value):
    """Perl prints 15 significant digits; x2x +af parses the text to a double and casts it."""
    return np.float32(float("%.15g" % value))


def rows(config_text, label_text, frame_shift):
    """The script's output as float32 [frames][features], and its warnings on stderr: (out of range, no state-level
    information)."""
    feats = parse_config(config_text)
    lines, level = parse_label(label_text, frame_shift)
    n = len(lines)
    first, last = list(range(n)), list(range(n))
    if level == "state":
        for i in range(n):
            a = b = i
            while a != 0 and lines[a - 1][3] < lines[a][3]:
                a -= 1
            while b != n - 1 and lines[b][3] < lines[b + 1][3]:
                b += 1
            first[i], last[i] = a, b
    out, out_of_range, no_state = [], 0, 0
    for i, (start, end, name, state) in enumerate(lines):
        fixed = []
        for fname, kind, patt, lo, hi in feats:
            v = 0.0
            if kind == "float":
                hit, value = match_number(name, patt)
                if hit:
                    ok, v = norm(value, lo, hi)
                    out_of_range += 0 if ok else 1
            elif kind == "binary":
                v = 1.0 if binary(name, patt) else 0.0
            fixed.append(as_float32(v))
        for j in range(start, end):
            row = list(fixed)
            for k, (fname, kind, patt, lo, hi) in enumerate(feats):
                if kind != "reserved":
                    continue
                which = RESERVED.index(fname)
                if which < 4 and level != "state":
                    no_state += 1
                    value = lo
                else:
                    value = (state, hi - state + lo, 1 + j - start, end - j, 1 + j - lines[first[i]][0],
                             lines[last[i]][1] - j)[which]
                ok, v = norm(value, lo, hi)
                out_of_range += 0 if ok else 1
                row[k] = as_float32(v)
            out.append(row)
    return np.asarray(out, dtype=np.float32).reshape(len(out), len(feats)), (out_of_range, no_state)
