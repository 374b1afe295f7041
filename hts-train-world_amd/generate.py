"""The recipe's generation stages as ONE pass over a batch: aligned labels in, waveforms out.

The reference runs them as separate steps (scripts/Training.pl:885-1015, PGEND / PGENT and WGEND / WGENT), and so do the
drivers of recipe.py, each of which reads the float32 files the one before it wrote:

    ffi_files          make_gen_data_dnn / makefeature.pl       labels            -> <base>.ffi
    forward_files      DNNSynthesis.py                          .ffi              -> <base>.ffo, <base>.var
    gen_param_files    gen_param / mlpg                         .ffo, .var        -> <base>.mgc, .lf0, .bap, ...
    postfilter_files   gen_wave, $pf == 1 (or mspf_files: 2)    .mgc              -> <base>.p_mgc
    synth_files        the WORLD `synth` CLI                    .lf0 .p_mgc .bap  -> <base>.wav

(With USEWORLD the reference's gen_wave stops after the postfilter: its two waveform branches are `!$usestraight &&
!$useworld`, scripts/Training.pl:2873, and `$usestraight`, :2900, so the recipe never calls `synth` itself.)

Generator holds what these steps share -- the compiled question config, the model, the speaker's variance row, the
windows, the postfilter's tables -- and runs the six library calls behind them on one WorldBatch, every step reading the
device tensors of the step before.  No kernel is its own: every call is the one the staged driver makes, with the
arguments the staged driver builds.  The float32 roundings of the staged files are kept where they are (MLPG's outputs are
float32; the postfilter's input is widened with .double() and its result rounded once with .float(); recipe_decode takes
float32), so the chain's waveform is the staged pipeline's, bit for bit -- not a more accurate one.

generate_files() is the file-list driver over it (`python -m hts-train-world_amd.recipe generate`).
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np

from . import modify as M, recipe as R, world as W

SYNTHESIS_STREAMS = ("mgc", "lf0", "bap")            # what recipe_decode and synthesize take; any other stream is returned only
FFT_SIZES = (512, 1024, 2048, 4096)                  # the sizes recipe_decode and synthesize are built for
STAGES = ("ffi", "forward", "mlpg", "postfilter")    # the status word's fields, 4 bits each, in this order
FFI_BITS, FORWARD_SHIFT, MLPG_SHIFT, POSTFILTER_SHIFT = 0xF, 4, 8, 12
GV_KEPT_MLPG = 4                                     # parameter_generation_gv: a column had no variance to work on; mlpg's stands


def y_length(n_frames, frame_period, fs):
    """Samples the synth CLI asks for n_frames frames (synth.cpp:259), as synth_files sizes its batch."""
    return int((n_frames - 1) * frame_period / 1000.0 * fs) + 1


def wav_size(n_samples):
    """Bytes of the file write_wav makes of n_samples samples: the 44-byte header and 16 bits each."""
    return 44 + 2 * int(n_samples)


def wav_complete(path, n_frames, frame_period, fs):
    """The test behind `resume`: the wav exists with the size write_wav gives the utterance's y_length samples."""
    return R._size_is(path, wav_size(y_length(n_frames, frame_period, fs)))


def label_frames(labels, names=None):
    """Frame counts of parsed labels (recipe.read_label); one without frames raises: a batch holds no empty utterance."""
    frames = [sum(e - s for s, e, _, _ in lines) for lines, _ in labels]
    for k, n in enumerate(frames):
        if n < 1:
            raise ValueError("%s holds %d frames, an utterance needs at least 1" % (names[k] if names else "label %d" % k, n))
    return frames


def status_word(ffi, forward, mlpg, postfilter):
    """One int32 per utterance of the four stages' own status values (arrays [n_utt]; postfilter already per utterance):
    ffi in bits 0-3, forward in 4-7, mlpg in 8-11, postfilter in 12-15."""
    word = np.asarray(ffi, dtype=np.int32) & FFI_BITS
    for shift, st in ((FORWARD_SHIFT, forward), (MLPG_SHIFT, mlpg), (POSTFILTER_SHIFT, postfilter)):
        word = word | ((np.asarray(st, dtype=np.int32) & 0xF) << shift)
    return word


def flagged_stage(word):
    """(stage name, that stage's status) of the first stage that flagged the utterance, or None: the ffi bits are
    warnings (a value was clamped; no state-level information), as in ffi_files, and so is GV generation's 4 in the
    mlpg field (an utterance of one frame, an unvoiced one: the trajectory is mlpg's, which is a waveform to use)."""
    for name, shift, bits in (("forward", FORWARD_SHIFT, 0xF), ("mlpg", MLPG_SHIFT, 0xF & ~GV_KEPT_MLPG),
                              ("postfilter", POSTFILTER_SHIFT, 0xF)):
        if (int(word) >> shift) & bits:
            return name, (int(word) >> shift) & bits
    return None


class _Setup:
    """The arguments of Generator, checked and loaded on the host: nothing here opens a context or touches a device."""

    def __init__(self, config, frame_shift, model, spkr=None, streams=(), fs=48000, frame_period=5.0, fft_size=2048,
                 alpha=0.55, postfilter=None, edge=0, unvoiced_value=-1.0e10, f0_scale=None, formant_ratio=None):
        from . import training
        self.names, self.features = R.read_question_config(config) if isinstance(config, (str, os.PathLike)) else config
        nf = len(self.features)
        if nf < 1:
            raise ValueError("the question config holds no feature")
        if int(frame_shift) < 1:
            raise ValueError("frame_shift must be positive, got %d" % int(frame_shift))
        self.frame_shift = int(frame_shift)
        self.model = training.AcousticModel.load(model) if isinstance(model, (str, os.PathLike)) else model
        if self.model.n_inputs != nf:
            raise ValueError("the model takes %d inputs, the question config yields %d features" % (self.model.n_inputs, nf))
        self.spkr = self.model.n_spkrs - 1 if spkr is None else int(spkr)
        if not 0 <= self.spkr < self.model.n_spkrs:
            raise ValueError("speaker %d: the model has %d" % (self.spkr, self.model.n_spkrs))
        streams = [tuple(s) for s in streams]
        if any(len(s) != 4 for s in streams):
            raise ValueError("a stream is (name, dim, windows, msd)")
        self.stream_names = [str(s[0]) for s in streams]
        self.streams = R._streams_arg([s[1:] for s in streams])
        self.layout, self.width = R.ffo_layout(self.streams)
        for name in SYNTHESIS_STREAMS:
            if self.stream_names.count(name) != 1:
                raise ValueError("stream %s is given %d times, synthesis needs it 1 time" % (name, self.stream_names.count(name)))
        if len(set(self.stream_names)) != len(self.stream_names):
            raise ValueError("%d streams carry %d names: a name is a file extension" % (len(streams), len(set(self.stream_names))))
        dim_of = lambda name: self.streams[self.stream_names.index(name)][0]
        lf0 = self.streams[self.stream_names.index("lf0")]
        if lf0[0] != 1 or not lf0[2]:
            raise ValueError("stream lf0 has dimension %d and msd %d: synthesis needs 1 and 1" % (lf0[0], int(lf0[2])))
        bap_order = dim_of("bap") - dim_of("bap") % 2                                  # synth.cpp:233-235
        if not 1 <= bap_order <= 63:
            raise ValueError("stream bap has dimension %d, its coding order %d is outside 1 .. 63" % (dim_of("bap"), bap_order))
        if self.model.n_outputs != self.width:
            raise ValueError("the model has %d outputs, an ffo row of these streams has %d" % (self.model.n_outputs, self.width))
        if int(fft_size) not in FFT_SIZES:
            raise ValueError("fft_size %d is not one of the supported %d ... %d (%s)" % (
                int(fft_size), FFT_SIZES[0], FFT_SIZES[-1], ", ".join(str(f) for f in FFT_SIZES)))
        self.fs, self.frame_period, self.fft_size = int(fs), float(frame_period), int(fft_size)
        self.alpha, self.edge, self.unvoiced_value = float(alpha), int(edge), float(unvoiced_value)
        for name, v in (("f0_scale", f0_scale), ("formant_ratio", formant_ratio)):
            if v is not None and np.ndim(v) != 0:
                raise ValueError("%s is one number for every utterance, got %r" % (name, v))
        M.factor_array("generate", "f0_scale", f0_scale, 1)
        M.factor_array("generate", "formant_ratio", formant_ratio, 1, self.fft_size)
        self.f0_scale = None if f0_scale is None else float(f0_scale)
        self.formant_ratio = None if formant_ratio is None else float(formant_ratio)
        if postfilter is not None and postfilter[0] == "gv":
            self.postfilter, self.tables = self._gv(postfilter, [d for d, _, _ in self.streams])
        else:
            self.postfilter, self.tables = self._postfilter(postfilter, dim_of("mgc"))

    @staticmethod
    def _gv(choice, dims):
        """("gv", gv_mean, gv_var, options): gv.mean and gv.var of gv_pdf_files (paths, or float32 rows over the static
        columns of all streams) and a dict of gen_param_gv_files' options.  Returns (("gv", options), per stream
        (gv_mean, gv_var))."""
        if len(choice) != 4:
            raise ValueError('postfilter ("gv", gv_mean, gv_var, options) takes three values, got %d' % (len(choice) - 1))
        options = dict(choice[3] or {})
        unknown = sorted(set(options) - set(R.GV_OPTIONS))
        if unknown:
            raise ValueError("postfilter gv: unknown option %s" % ", ".join(unknown))
        rows = [np.fromfile(str(a), dtype=np.float32) if isinstance(a, (str, os.PathLike)) else np.asarray(a, dtype=np.float32)
                for a in choice[1:3]]
        for what, r in zip(("gv_mean", "gv_var"), rows):
            if r.shape != (sum(dims),):
                raise ValueError("postfilter gv: %s holds %d values, the streams have %d static columns" % (what, r.size, sum(dims)))
        at = np.concatenate([[0], np.cumsum(dims)])
        return ("gv", options), [(rows[0][at[k]:at[k + 1]], rows[1][at[k]:at[k + 1]]) for k in range(len(dims))]

    @staticmethod
    def _postfilter(choice, dim):
        """None, ("mcp", beta, length) or ("mspf", emphasis, frame_length, fft_length) and, for mspf, the four tables
        float64 [dim][fft_length / 2 + 1] as mspf_files reads them."""
        if choice is None:
            return None, None
        kind = choice[0]
        if kind == "mcp" and len(choice) == 3:
            return ("mcp", float(choice[1]), int(choice[2])), None
        if kind == "mspf" and len(choice) == 6:
            _, gen_dir, nat_dir, emphasis, frame_length, fft_length = choice
            K = int(fft_length) // 2 + 1

            def table(directory, which):
                rows = [np.fromfile(R._mspf_stat_paths(directory, "mgc", d)[which], dtype=np.float32) for d in range(dim)]
                for d, r in enumerate(rows):
                    if len(r) != K:
                        raise ValueError("%s holds %d bins, fft_length %d needs %d" % (
                            R._mspf_stat_paths(directory, "mgc", d)[which], len(r), int(fft_length), K))
                return np.stack(rows).astype(np.float64)

            tables = (table(gen_dir, 0), table(gen_dir, 1), table(nat_dir, 0), table(nat_dir, 1))
            return ("mspf", float(emphasis), int(frame_length), int(fft_length)), tables
        raise ValueError('postfilter is None, ("mcp", beta, length), ("mspf", gen_stats_dir, nat_stats_dir, emphasis, '
                         'frame_length, fft_length) or ("gv", gv_mean, gv_var, options)')


class Generated:
    """What one Generator call leaves, all of it on the device (n_utt utterances back to back, as the batch holds them):

    y        float64 [total_out], the waveforms; pcm: int16 [total_out], the samples write_wav stores (samples_to_pcm16)
    streams  {name: float32 [total_frames][dim]} as MLPG left them; p_mgc: the postfiltered mgc, or None without one
    ffi, ffo float32 [total_frames][n_inputs], [total_frames][n_outputs]: the model's input and output rows
    status   numpy int32 [n_utt], status_word(); flagged: {utterance: (stage name, its status)} -- the waveform of a
             flagged utterance is not to be used
    frame_offsets, out_offsets: numpy [n_utt + 1], where an utterance's rows and samples start."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def rows(self, t, k):
        return t[int(self.frame_offsets[k]):int(self.frame_offsets[k + 1])]

    def waveform(self, k):
        return self.y[int(self.out_offsets[k]):int(self.out_offsets[k + 1])]

    def samples(self, k):
        return self.pcm[int(self.out_offsets[k]):int(self.out_offsets[k + 1])]


class Generator:
    """Aligned labels to waveforms on one device-resident batch per call; built once, called many times.

        gen = Generator(config, frame_shift, model_npz, spkr, streams, fs, frame_period, fft_size, alpha, postfilter)
        out = gen([read_label(p, frame_shift) for p in paths])        # a Generated
        gen.close()

    config:      the question config's path, or what recipe.parse_question_config returned
    frame_shift: one frame in the labels' time unit of 100 ns, as ffi_files takes it
    model:       the `.npz` of training.AcousticModel.save (or such a module); spkr: None for its last speaker
    streams:     [(name, dim, windows, msd)] in the ffo row's order, windows as gen_param_files takes them; the streams
                 named mgc, lf0 and bap feed synthesis, any other (vib) is generated and returned
    postfilter:  None, ("mcp", beta, length) -- postfilter_files on the mgc stream at `alpha` --, or ("mspf",
                 gen_stats_dir, nat_stats_dir, emphasis, frame_length, fft_length) -- mspf_files on mgc_dim<d>.mean / .stdd
                 --, or ("gv", gv_mean, gv_var, options) -- gen_param_gv_files' generation in MLPG's place and, as gen_wave
                 does with GV generation on, no postfilter after it; its status is the status word's mlpg field
    edge, unvoiced_value: as gen_param_files
    f0_scale, formant_ratio: None, or a pitch and a formant knob (modify.modify_features) on the decoded f0 and spectral
                 envelope, between recipe_decode and synthesize; with both None no such call is made
    ctx:         a world.Context, or None for one of its own (closed by close()).  The casts between the library's calls
                 are torch's: with a context on a caller's stream, call with that stream as torch's current one.

    Held on the device between calls: the LabelFeatureSet, the model, the speaker's variance row (float32, the row
    forward_files writes as <base>.var).  The windows and the four MSPF tables stay on the host, float64, as
    parameter_generation and postfilter_modulation_spectrum take them: the library uploads them itself with every call.
    Every argument is checked before a context is opened; each check raises ValueError with the numbers that disagree."""

    def __init__(self, config, *args, ctx=None, **kwargs):
        import torch
        s = config if isinstance(config, _Setup) else _Setup(config, *args, **kwargs)
        self.setup = s
        self.own_ctx = ctx is None
        self.ctx = ctx or R._own_context()
        self.fset = None
        try:
            self.fset = W.LabelFeatureSet(self.ctx, s.features)
            self.model = s.model.cuda()
            self.var_row = self.model.variance.variances[s.spkr].detach().to(torch.float32)       # forward_files' var_row
            self.params = W.default_params(s.fs, s.frame_period, fft_size=s.fft_size)              # synth_files' params
            self.gv = None
            if s.postfilter and s.postfilter[0] == "gv":                                           # gen_param_gv_files' rows
                self.gv = ([R._upload(m) for m, _ in s.tables], [R._upload(v) for _, v in s.tables])
        except BaseException:
            self.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *_):
        self.close()

    def close(self):
        if self.fset is not None:
            self.fset.close()
            self.fset = None
        if self.own_ctx and self.ctx is not None:
            self.ctx.close()
        self.ctx = None

    def __call__(self, labels, names=None, pcm=True, report=True):
        """labels: [(lines, state_level)] as recipe.read_label returns them; names: what to call them on stderr.  Runs
        label_features, AcousticModel.infer, parameter_generation, the postfilter, recipe_decode and synthesize on one
        WorldBatch whose f0_lengths are the labels' frame counts and whose y_lengths are y_length() of them; the
        statuses come to the host after the last launch.  An utterance flagged by the forward pass, MLPG or the
        postfilter is reported once on stderr (report=False: not) and named in Generated.flagged; nothing raises for it."""
        s = self.setup
        frames = label_frames(labels, names)
        with contextlib.closing(W.WorldBatch(self.ctx, self.params, f0_lengths=frames,
                                             y_lengths=[y_length(t, s.frame_period, s.fs) for t in frames])) as b:
            ffi, st_ffi = b.label_features(self.fset, labels)                                       # ffi_files
            ffo, _, st_fwd = self.model.infer(b, ffi, [s.spkr] * len(frames))                       # forward_files
            args = [(ffo[:, c0:c0 + n], self.var_row[c0:c0 + n], wins, None if mcol is None else ffo[:, mcol])
                    for (mcol, c0, n), (_, wins, _) in zip(s.layout, s.streams)]                    # gen_param_files
            if self.gv is not None:                                                                 # gen_param_gv_files
                outs, st_mlpg = b.parameter_generation_gv(args, self.gv[0], self.gv[1], edge=s.edge,
                                                          unvoiced_value=s.unvoiced_value, **s.postfilter[1])
            else:
                outs, st_mlpg = b.parameter_generation(args, edge=s.edge, unvoiced_value=s.unvoiced_value)
            gen = dict(zip(s.stream_names, outs))
            p_mgc, st_post = None, None
            if s.postfilter and s.postfilter[0] == "mcp":                                           # postfilter_files
                out, st_post = b.postfilter_mel_cepstrum(gen["mgc"].double(), s.alpha, s.postfilter[1], s.postfilter[2])
                p_mgc = out.float()
            elif s.postfilter and s.postfilter[0] == "mspf":                                        # mspf_files; gv: none (gen_wave:749-757)
                out, st_post = b.postfilter_modulation_spectrum(gen["mgc"].double(), *s.tables, *s.postfilter[1:])
                p_mgc = out.float()
            f0, sp, ap = b.recipe_decode(gen["lf0"].reshape(-1), gen["mgc"] if p_mgc is None else p_mgc, gen["bap"])
            if s.f0_scale is not None or s.formant_ratio is not None:                               # test.cpp:201-238
                f0, sp = M.modify_features(b, f0, sp, s.f0_scale, s.formant_ratio, out=(f0, sp))
            y = b.synthesize(f0, sp, ap)                                                            # synth_files
            del f0, sp, ap
            samples = b.samples_to_pcm16(y) if pcm else None
            fo, yo = b.frame_offsets, b.out_offsets
            post = np.zeros(len(frames), dtype=np.int32)
            if st_post is not None:
                post = st_post.cpu().numpy()
                if s.postfilter[0] == "mcp":                                                        # per frame: any of them
                    post = np.bitwise_or.reduceat(post, fo[:-1].astype(np.intp))
            word = status_word(st_ffi.cpu().numpy(), st_fwd.cpu().numpy(), st_mlpg.cpu().numpy(), post)
        flagged = {k: flagged_stage(w) for k, w in enumerate(word) if flagged_stage(w)}
        if report:
            for k, (stage, st) in flagged.items():
                print("warning: %s: flagged by %s (status %d), no waveform" % (names[k] if names else "utterance %d" % k,
                                                                              stage, st), file=sys.stderr)
        return Generated(y=y, pcm=samples, streams=gen, p_mgc=p_mgc, ffi=ffi, ffo=ffo, status=word, flagged=flagged,
                         frame_offsets=fo, out_offsets=yo, frames=frames)


def generate_files(jobs, config, frame_shift, model, spkr=None, streams=(), fs=48000, frame_period=5.0, fft_size=2048,
                   alpha=0.55, postfilter=None, edge=0, unvoiced_value=-1.0e10, ctx=None, keep_dir=None,
                   max_batch_frames=R.MAX_BATCH_FRAMES, io_threads=8, resume=False, f0_scale=None, formant_ratio=None):
    """Labels to wavs for a file list: ffi_files, forward_files, gen_param_files, postfilter_files or mspf_files, and
    synth_files as one pass per batch (Generator, whose arguments these are), with no file between them.

    jobs:     [(label_file, wav_out)]; the wav is write_wav's, as synth_files writes it
    keep_dir: None, or where to leave what the staged commands would have left, with the same bytes, under the label
              file's base name: <base>.ffi, <base>.ffo, <base>.var, <base>.<stream> for every stream, and <base>.p_mgc
              when a postfilter ran
    resume:   skip a job whose wav exists with the size write_wav gives its samples (wav_complete)
    f0_scale, formant_ratio: Generator's; the kept files are the unmodified features' either way
    Rank-sharded by frame count.  An utterance flagged by the forward pass, MLPG or the postfilter is reported on stderr
    with the stage's name and gets no wav (its kept files are written, flagged rows being zeros as the stages leave them);
    the ffi warnings are counted as ffi_files counts them.  Every argument is checked before a context is opened.
    Returns (frames generated by this rank, [(label_file, stage, status)] of its flagged utterances)."""
    jobs = [tuple(j) for j in jobs]
    if any(len(j) != 2 for j in jobs):
        raise ValueError("generate_files: a job is (label_file, wav_out)")
    setup = _Setup(config, frame_shift, model, spkr, streams, fs, frame_period, fft_size, alpha, postfilter, edge,
                   unvoiced_value, f0_scale, formant_ratio)
    labels = [R.read_label(j[0], setup.frame_shift) for j in jobs]
    frames = label_frames(labels, [j[0] for j in jobs])
    mine = R._my_jobs(frames, lambda i: not (resume and wav_complete(jobs[i][1], frames[i], setup.frame_period, setup.fs)))
    if not mine:
        return 0, []
    bases = [None if keep_dir is None else os.path.join(str(keep_dir), os.path.splitext(os.path.basename(j[0]))[0])
             for j in jobs]
    flagged, clamped, no_state = [], 0, 0
    with R._Stage(ctx, io_threads) as stage, Generator(setup, ctx=stage.ctx) as gen:
        var_row = gen.var_row.cpu().numpy() if keep_dir is not None else None
        if keep_dir is not None:
            os.makedirs(str(keep_dir), exist_ok=True)
        for group in stage.groups(mine, frames, max_batch_frames):
            out = gen([labels[i] for i in group], [jobs[i][0] for i in group], pcm=False)
            stage.frames += sum(out.frames)
            y = out.y.cpu().numpy()
            for k, i in enumerate(group):
                if k in out.flagged:
                    flagged.append((jobs[i][0],) + out.flagged[k])
                else:
                    stage.submit(R.write_wav, jobs[i][1], y[out.out_offsets[k]:out.out_offsets[k + 1]], setup.fs)
            clamped += int((out.status & 1 != 0).sum())
            no_state += int((out.status & 2 != 0).sum())
            if keep_dir is not None:
                kept = [("ffi", out.ffi), ("ffo", out.ffo)] + list(out.streams.items())
                if out.p_mgc is not None:
                    kept.append(("p_mgc", out.p_mgc))
                stage.put_native(out, [(t.cpu().numpy(), [bases[i] + "." + ext for i in group]) for ext, t in kept], io_threads)
                for i in group:
                    stage.submit(var_row.tofile, bases[i] + ".var")
    print("warnings: Out of range in %d utterances, no state-level information in %d" % (clamped, no_state), file=sys.stderr)
    return stage.frames, flagged
