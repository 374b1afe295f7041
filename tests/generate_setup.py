"""The small world of the `generate` tests: a question config and label names taken from the makefeature.pl fixture
(tests/golden/label_features.npz, as tests/test_recipe_ffi.py uses it), four aligned label files, and an acoustic model
whose weights are set by hand around a seeded generator -- 16 kHz, 5 ms frames, fft_size 512, four streams with the
recipe's three windows each, an ffo row of 34 columns.

The model (9 inputs, one hidden layer of 8 sigmoid units, 34 linear outputs):
  unit 0      follows C-vowel alone (sigmoid(+-2)); the voicing column is that unit plus a little of the others, so vowels
              are voiced, everything else is not: both kinds of frames, and utterances without a vowel are unvoiced whole
  units 1-5   seeded weights on every feature
  units 6, 7  fire on the name `zz` alone (sigmoid(+-500): exactly 1 or 0 in float32) and weigh 3e38 each on output
              column 0: an utterance that holds a `zz` overflows float32 there and is flagged by the forward pass ("a
              non-finite output"), an utterance without one receives exactly 0 from them.  No clean label holds a `zz`.
The lf0 mean is ln 180 plus at most a few tenths, and the variances of the dynamic columns are a hundred times the static
ones', so that the trajectory stays near the static means also at an utterance's ends, where SPTK's mlpg (edge 0) drops
the window taps beyond them and the dynamic rows pull the last frames towards 0: lf0 stays between ln 80 and ln 400."""
import os

import numpy as np

from conftest import GOLDEN

FS, FRAME_PERIOD, FRAME_SHIFT, FFT_SIZE = 16000, 5.0, 50000, 512
ALPHA = 0.42
WINDOWS = [[1.0], [-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]
STREAMS = [("mgc", 6, WINDOWS, False), ("lf0", 1, WINDOWS, True), ("bap", 2, WINDOWS, False), ("vib", 2, WINDOWS, False)]
WIDTH = 34
# the shortest utterance every staged driver accepts (tests/test_gpu_mlpg.py LENGTHS[0]), one without a vowel, 97, about 160
LENGTHS = (1, 33, 97, 161)
CONFIG_NAMES = ("C-sil", "C-pau", "C-vowel", "C-nasal", "A1", "A2", "D-after-plus", "Pos_C-Frame_in_Phone(Fw)")
TRIGGER = "C-zz             {*-zz+*}"
N_INPUTS, UNITS = len(CONFIG_NAMES) + 1, 8
MSD_COLUMN, LF0_COLUMN = 18, 19
POSTFILTERS = ("none", "mcp", "mspf")
MCP = ("mcp", 1.4, 1024)
MSPF = (1.0, 25, 64)                                 # emphasis, frame_length, fft_length


def config_text():
    """The fixture's lines of CONFIG_NAMES, in that order, and the trigger feature."""
    fx = np.load(os.path.join(GOLDEN, "label_features.npz"))
    lines = {ln.split()[0]: ln for ln in str(fx["recipe/config"]).split("\n") if ln.strip() and not ln.startswith("#")}
    return "\n".join([lines[n] for n in CONFIG_NAMES] + [TRIGGER]) + "\n"


def phone_names():
    """The ten phoneme-level names of the fixture's fourth label file, (vowels, others)."""
    fx = np.load(os.path.join(GOLDEN, "label_features.npz"))
    names = [ln.split()[2] for ln in str(fx["recipe/label3"]).split("\n") if ln.strip()]
    is_vowel = lambda n: any("-%s+" % v in n for v in "aiueo")
    return [n for n in names if is_vowel(n)], [n for n in names if not is_vowel(n)]


def label_text(n_frames, names, rng):
    """n_frames frames cut into len(names) or fewer segments of seeded lengths, one name each, in 100 ns units."""
    k = min(len(names), n_frames)
    cuts = np.sort(rng.choice(np.arange(1, n_frames), size=k - 1, replace=False)) if k > 1 else np.zeros(0, dtype=int)
    edges = np.concatenate([[0], cuts, [n_frames]]).astype(int)
    return "".join("%d %d %s\n" % (edges[i] * FRAME_SHIFT, edges[i + 1] * FRAME_SHIFT, names[i]) for i in range(k))


def label_texts(seed=5):
    """The four clean utterances of LENGTHS: [a silence of one frame, no vowel at all, every name, every name]."""
    vowels, others = phone_names()
    every = [n for pair in zip(others, vowels + vowels) for n in pair]
    rng = np.random.default_rng(seed)
    return [label_text(LENGTHS[0], [n for n in others if "-sil+" in n], rng), label_text(LENGTHS[1], others, rng),
            label_text(LENGTHS[2], every, rng), label_text(LENGTHS[3], every[::-1], rng)]


def flagged_label_text(n_frames=40, seed=6):
    """An utterance with one `zz` among its names: the forward pass flags it."""
    vowels, others = phone_names()
    return label_text(n_frames, [others[0], vowels[0], "x^x-zz+x=x/A:0+0_00/B:1@1/C:b/D:+0|x$f/E:_0_0_0", vowels[1]],
                      np.random.default_rng(seed))


def model_arrays(n_spkrs, seed=7):
    """The state of the model in the module's docstring, float32, under training.AcousticModel's names."""
    rng = np.random.default_rng(seed)
    w0 = rng.normal(0.0, 0.5, (N_INPUTS, UNITS))
    b0 = rng.normal(0.0, 0.2, UNITS)
    w0[:, 0], w0[2, 0], b0[0] = 0.0, 4.0, -2.0
    w0[:, 6:8], w0[N_INPUTS - 1, 6:8], b0[6:8] = 0.0, 1000.0, -500.0
    w0[N_INPUTS - 1, :6] = 0.0
    w1 = rng.normal(0.0, 0.2, (UNITS, WIDTH))
    b1 = rng.normal(0.0, 0.1, WIDTH)
    b1[:6] += (0.5, 0.3, 0.1, 0.05, 0.0, 0.0)
    w1[:, MSD_COLUMN], w1[0, MSD_COLUMN], b1[MSD_COLUMN] = rng.normal(0.0, 0.02, UNITS), 1.0, 0.0
    w1[:, LF0_COLUMN], b1[LF0_COLUMN] = rng.normal(0.0, 0.1, UNITS), np.log(180.0)
    w1[:, LF0_COLUMN + 1:LF0_COLUMN + 3], b1[LF0_COLUMN + 1:LF0_COLUMN + 3] = rng.normal(0.0, 0.01, (UNITS, 2)), 0.0
    w1[6:8, :], w1[6:8, 0] = 0.0, 3.0e38
    var = rng.uniform(0.5, 2.0, (n_spkrs, WIDTH))
    at = 0
    for _, dim, wins, msd in STREAMS:                  # the dynamic columns a hundred times wider than the static ones
        at += 1 if msd else 0
        var[:, at + dim:at + dim * len(wins)] *= 100.0
        at += dim * len(wins)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    arrays = {"hidden0.si_weights": f(w0), "hidden0.si_biases": f(b0), "output.si_weights": f(w1), "output.si_biases": f(b1),
              "variance.variances": f(var)}
    if n_spkrs > 1:
        arrays["hidden0.sd_weights"] = f(rng.normal(0.0, 0.3, (n_spkrs, UNITS)))
    return arrays


def save_model(pkg, path, n_spkrs=1):
    import torch
    m = pkg.training.AcousticModel(N_INPUTS, [UNITS], WIDTH, n_spkrs, "sigmoid", "linear")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in model_arrays(n_spkrs).items()})
    m.save(str(path))
    return str(path)


def write_mspf_tables(directory, shift, seed=8):
    """mgc_dim<d>.mean / .stdd of the mgc stream, fft_length / 2 + 1 float32 each, from the seeded generator; `shift`
    moves the natural side a little off the generated one."""
    os.makedirs(str(directory), exist_ok=True)
    rng = np.random.default_rng(seed)
    K = MSPF[2] // 2 + 1
    for d in range(STREAMS[0][1]):
        mean, std = rng.normal(0.0, 1.0, K), rng.uniform(0.5, 1.5, K)
        base = os.path.join(str(directory), "mgc_dim%d" % d)
        (mean + shift * rng.normal(0.0, 1.0, K)).astype(np.float32).tofile(base + ".mean")
        (std * (1.0 + shift * rng.uniform(0.0, 1.0, K))).astype(np.float32).tofile(base + ".stdd")
    return str(directory)


class World:
    """The files of the setup under `root`: q.conf, a<k>.lab, sd.npz, sat.npz, stats/gen and stats/nat."""

    def __init__(self, pkg, root):
        self.root = str(root)
        self.config = os.path.join(self.root, "q.conf")
        with open(self.config, "w") as f:
            f.write(config_text())
        self.labels = []
        for k, text in enumerate(label_texts()):
            self.labels.append(os.path.join(self.root, "a%d.lab" % k))
            with open(self.labels[-1], "w") as f:
                f.write(text)
        self.flagged_label = os.path.join(self.root, "z0.lab")
        with open(self.flagged_label, "w") as f:
            f.write(flagged_label_text())
        self.models = {"sd": (save_model(pkg, os.path.join(self.root, "sd.npz"), 1), None),
                       "sat": (save_model(pkg, os.path.join(self.root, "sat.npz"), 3), 0)}
        self.gen_stats = write_mspf_tables(os.path.join(self.root, "stats", "gen"), 0.0)
        self.nat_stats = write_mspf_tables(os.path.join(self.root, "stats", "nat"), 0.1)

    def postfilter(self, which):
        return {"none": None, "mcp": MCP, "mspf": ("mspf", self.gen_stats, self.nat_stats) + MSPF}[which]

    def arguments(self, which="mcp", kind="sd"):
        """generate_files' / Generator's arguments after the job list or in front of ctx."""
        model, spkr = self.models[kind]
        return dict(config=self.config, frame_shift=FRAME_SHIFT, model=model, spkr=spkr, streams=STREAMS, fs=FS,
                    frame_period=FRAME_PERIOD, fft_size=FFT_SIZE, alpha=ALPHA, postfilter=self.postfilter(which))

    def staged(self, R, out_dir, which="mcp", kind="sd", labels=None, ctx=None):
        """ffi_files -> forward_files -> gen_param_files -> (postfilter_files | mspf_files | nothing) -> synth_files into
        out_dir, every stage on its defaults.  Returns the base paths."""
        labels = self.labels if labels is None else labels
        os.makedirs(str(out_dir), exist_ok=True)
        model, spkr = self.models[kind]
        base = [os.path.join(str(out_dir), os.path.splitext(os.path.basename(p))[0]) for p in labels]
        names = [s[0] for s in STREAMS]
        R.ffi_files([(p, b + ".ffi") for p, b in zip(labels, base)], self.config, FRAME_SHIFT, ctx=ctx)
        R.forward_files([(b + ".ffi", None) for b in base], model, str(out_dir), spkr=spkr, ctx=ctx)
        R.gen_param_files([(b + ".ffo",) + tuple(b + "." + n for n in names) for b in base], [s[1:] for s in STREAMS],
                          base[0] + ".var", ctx=ctx)
        mgc = ".mgc"
        if which == "mcp":
            R.postfilter_files([(b + ".mgc", b + ".p_mgc") for b in base], STREAMS[0][1] - 1, ALPHA, MCP[1], MCP[2], ctx=ctx)
            mgc = ".p_mgc"
        elif which == "mspf":
            R.mspf_files([(b + ".mgc", b + ".p_mgc") for b in base], STREAMS[0][1], self.gen_stats, self.nat_stats, "mgc",
                         *MSPF, ctx=ctx)
            mgc = ".p_mgc"
        R.synth_files([(b + ".lf0", b + mgc, b + ".bap", b + ".wav") for b in base], FRAME_PERIOD, FFT_SIZE, FS,
                      STREAMS[0][1], STREAMS[2][1], ctx=ctx)
        return base

    @staticmethod
    def extensions(which):
        return ["ffi", "ffo", "var"] + [s[0] for s in STREAMS] + (["p_mgc"] if which != "none" else [])
