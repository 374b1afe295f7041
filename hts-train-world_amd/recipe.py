"""Batched stand-in for the recipe's per-utterance loops around the two CLIs.

The reference runs one process per utterance (data/Makefile.in:206-216):

    analysis  WAV  LF0  MGC  BAP  [frame_period [fft_size [spec_dim [ap_dim]]]]   (test/analysis.cpp:243-390)
    synth     LF0  MGC  BAP  WAV  frame_period fft_size fs [spec_dim [ap_dim]]    (test/synth.cpp:124-262)

Here a whole file list is read, packed into HBM-resident batches, analysed or synthesised in one set of
launches per batch, and written back in the CLIs' own file formats (SURVEY.md 8(b) "File contract"):

    wav in      16-bit mono PCM, x = s / 2^(nbit-1)                       (test/audioio.cpp:236-249)
    f0 / lf0    float32 [T]            Hz, or log Hz with 0 for unvoiced when spec_dim != 0
    sp / mgc    float32 [T][F/2+1]     or [T][spec_dim] coded
    ap / bap    float32 [T][F/2+1]     or [T][ap_dim] coded
    wav out     16-bit mono PCM, s = clip(int(y * 32767))                 (test/audioio.cpp:160-167)

Settings are the CLI's: Dio(71-800 Hz, speed 1, allowed_range 0.1) + StoneMask, CheapTrick(q1 -0.15),
D4C(threshold 0) (analysis.cpp:93-203).  `--f0 harvest` puts Harvest in Dio's place (`--no-refine`: without StoneMask
behind it), `--f0-floor` / `--f0-ceil` set the estimator's search range; the files keep their layout.  With several ranks (torch.distributed initialised, or WORLD_SIZE in
the environment) the list is sharded by frame count (sharding.lpt_shards; the counts come from the wav headers, a rank decodes only
its own utterances) and every rank writes its own files, or -- `--gather`, BASELINE.json configs[3] -- the float32
features travel to rank 0, which writes them all.

    python -m hts-train-world_amd.recipe analysis --scp jobs.txt --frame-period 5 --fft-size 2048 \\
           --spec-dim 50 --ap-dim 25          # jobs.txt: one "wav f0 sp ap" per line
    python -m hts-train-world_amd.recipe synth --scp jobs.txt --frame-period 5 --fft-size 2048 --fs 48000 \\
           --spec-dim 50 --ap-dim 25          # jobs.txt: one "f0 sp ap wav" per line

cmp_files() is the stage after it (data/Makefile.in:244-323: window.pl per stream, merge, addhtkheader.pl).
gv_pdf_files() / `gv-pdf` and gen_param_gv_files() / `gen-param-gv` are gen-param for a voice trained with GV: the pdf
of the per-utterance variances that `gv-data` writes, and parameter generation that also maximises its likelihood
(HMGenS with USEHMMGV = 1, scripts/Training.pl:1892-1903), after which gen_wave skips the postfilter (:749-757).
gen_param_files() / `gen-param` is the first stage of the way back (scripts/Training.pl:2755-2810: SPTK mlpg on a
model's `ffo` rows), in front of synth.  postfilter_files() / `postfilter` is the step gen_wave takes between the two
(scripts/Training.pl:2642-2687, postfiltering_mcp: `.mgc` in, `.p_mgc` out).  With GAMMA != 0 gen_wave's
`mgc2mgc` steps (:2861-2868; postfiltering_lsp's :2702-2705) are mgc2mgc_files() / `mgc2mgc`; the whole line from MGC-LSP
rows, `lspcheck | lsp2lpc | mgc2mgc -n -u`, is lsp2mgc_files() / `lsp2mgc`, and postfiltering_lsp (:2690-2752) is
postfilter_lsp_files() / `postfilter-lsp`.  With USEMSPF gen_wave takes
postfiltering_mspf instead (:2950-3038): mspf_files() / `mspf`, on the statistics files that mspf_stats_files() /
`mspf-stats` write (make_mspf, :3133-3221).
mgcep_files() / `mgcep` is the recipe's spectral analysis without WORLD (data/Makefile.in:134-137, the default
USEWORLD=0, GAMMA=0): `x2x +sf | frame | window | mgcep` from raw or wav files to float32 mgc, one kernel per batch.

trajectory_files() / `trj-eval` stands where gen_param_files() stands when the model was trained by trajectory training
($TRJGV, scripts/Training.pl:930-940): the outputs and the cost of DNNDefine.trajectory_cost; the loss itself, for a
torch model, is training.TrajectoryLoss.

train_files() / `dnn-train` is DNNTraining.py (SD, SAT and with --adapt ADAPT; frame by frame, or with --stream trajectory
training) on the library's training pass; with --updates tf1 the step itself is the library's too (Tf1Optimizer: TF 1.x's
update rules in one launch, the optimiser's state saved with the model).
forward_files() / `dnn-forward` is the step in front of both (scripts/Training.pl:877, 906, 964, 993: DNNSynthesis.py
frame by frame): the acoustic model's outputs for a list of `.ffi` files, the speaker's variance row and, where the
targets are paired, the cost.

The way out goes on after `cmp` (the reference's `analysis` target is `features cmp ffo stats`, data/Makefile.in:117):
ffo_files() / `ffo` writes the frame-by-frame training targets (:325-412: interpolate.pl on the msd stream, its voicing
flag, window.pl, merge), stats_files() / `stats` the variances gen_param_files() reads and the GV of the corpus
(:414-459), gv_data_files() / `gv-data` the per-utterance variance vectors of GV training (make_data_gv,
scripts/Training.pl:1402-1491).  ffi_files() / `ffi` writes the other side of the training pairs, the acoustic model's
input rows from aligned labels and a question config (make_train_data_dnn / make_gen_data_dnn, :1677-1723:
data/scripts/makefeature.pl and x2x +af), which `dnn-train`, `dnn-forward` and `trj-eval` read.

modify_files() / `modify` is the reference's own example program (test/test.cpp: `test in.wav out.wav [f0_scale
[formant_ratio]]`) for a file list: analysis, F0 scaling and formant shift (modify.py, test.cpp:201-238), synthesis, wav
to wav on the device.

generate_files() / `generate` (generate.py) is the way back in one pass: `ffi`, `dnn-forward`, `gen-param`, the postfilter
and `synth` on one device-resident batch, labels in and wavs out, with the staged commands' bytes.

There is no CPU path: without a HIP device the library call fails.
"""
from __future__ import annotations

import argparse
import contextlib
import math
import os
import re
import struct
import sys
import wave
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import capi, sharding, world as W

MAX_BATCH_FRAMES = 1_500_000          # about 12.3 GB of fp64 sp + ap at F = 1024; far inside 288 GB


# ---- file formats -----------------------------------------------------------------------------------------
def read_wav(path):
    """x in [-1, 1) and fs, as test/audioio.cpp wavread() hands them over (little-endian two's complement
    of nbit bits over 2^(nbit-1); the first channel layout is taken as it is: the CLIs assume mono)."""
    with wave.open(str(path), "rb") as w:
        nbytes, fs, n = w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    if nbytes == 2:
        s = np.frombuffer(raw, dtype="<i2").astype(np.float64)
    else:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, nbytes).astype(np.int64)
        s = sum(b[:, k] << (8 * k) for k in range(nbytes))
        s = np.where(s >= 1 << (8 * nbytes - 1), s - (1 << (8 * nbytes)), s).astype(np.float64)
    return s / float(1 << (8 * nbytes - 1)), fs


def write_wav(path, y, fs):
    """test/audioio.cpp wavwrite(): 44-byte header, int16 = clip(trunc(y * 32767))."""
    s = np.clip(np.trunc(np.asarray(y, dtype=np.float64) * 32767.0), -32768, 32767).astype("<i2")
    n = len(s)
    head = b"RIFF" + struct.pack("<I", 36 + n * 2) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, fs, fs * 2, 2, 16)
    with open(path, "wb") as f:
        f.write(head + b"data" + struct.pack("<I", n * 2))
        f.write(s.tobytes())


def _f32(path, cols=None):
    a = np.fromfile(path, dtype=np.float32)
    return a if cols is None else a.reshape(-1, cols)


# ---- batching ---------------------------------------------------------------------------------------------
def _my_share(costs):
    """Indices of this rank's jobs (all of them on a single process)."""
    rank, world = _rank_world()
    if world == 1:
        return list(range(len(costs)))
    return sharding.lpt_shards(costs, world)[rank]


def _own_context():
    """A context on this rank's GPU (LOCAL_RANK of a torchrun launch, else the current device)."""
    import torch
    local = os.environ.get("LOCAL_RANK")
    if local is not None:
        torch.cuda.set_device(int(local))
        return W.Context(device=int(local))
    return W.Context()


def _batches(order, frames, limit, fits=None):
    """Groups of `order` within `limit` frames and, where given, fits(group) (sweep.batches: the same rule)."""
    cur, tot = [], 0
    for i in order:
        if cur and (tot + frames[i] > limit or (fits is not None and not fits(cur + [i]))):
            yield cur
            cur, tot = [], 0
        cur.append(i)
        tot += frames[i]
    if cur:
        yield cur


def _size_is(path, size):
    try:
        return os.path.getsize(str(path)) == size
    except OSError:
        return False


def _rows_in(job, width, n_paths=None, what=None):
    """Frames of `job` from the size of its first file, rows of `width` float32; with n_paths the job must hold that
    many paths, which `what` names in the error."""
    size = os.path.getsize(job[0])
    if (n_paths is not None and len(job) != n_paths) or size % (4 * width):
        raise ValueError("%s: %d bytes are no rows of %d float32%s" % (job[0], size, width, ", or not " + what if what else ""))
    return size // (4 * width)


def _my_jobs(frames, todo=lambda i: True):
    """This rank's share of the jobs i with todo(i): the partition by frame count is made on those alone."""
    left = [i for i in range(len(frames)) if todo(i)]
    return [left[k] for k in _my_share([frames[i] for i in left])]


def _upload(a, pinned=False):
    """One host array as a device tensor: the drivers' only way onto the GPU."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.pin_memory().cuda(non_blocking=True) if pinned else t.cuda()


def _put(path, rows, head=None):
    if head is None:
        np.ascontiguousarray(rows).tofile(path)
    else:
        with open(path, "wb") as f:
            f.write(head)
            f.write(np.ascontiguousarray(rows).tobytes())


def _row_slices(b, host, paths):
    """[(path, the rows of utterance k of batch `b` in the slab `host`)] for paths[k] that are not None: row slices of
    a contiguous slab, contiguous themselves."""
    fo = b.frame_offsets
    return [(p, host[fo[k]:fo[k + 1]]) for k, p in enumerate(paths) if p is not None]


class _Stage:
    """What a file-list driver holds open: the context (its own when the caller gave none), the threads that read and
    write files, and the writes in flight.  Leaving it waits for every write that was submitted; then, after a body
    that did not raise, the first write that failed raises; a context made here is closed either way, a caller's never.
    `frames` adds up the frames of the batches opened.  A driver opens it ahead of its first call into the library:
    _own_context imports torch first (analysis_files says why)."""

    def __init__(self, ctx, io_threads):
        self.pool = ThreadPoolExecutor(io_threads)
        self.writes, self.frames = [], 0
        self.own_ctx = ctx is None
        self.ctx = ctx or _own_context()

    def __enter__(self):
        return self

    def __exit__(self, failed, *_):
        try:
            self.pool.shutdown(wait=True)
            if failed is None:
                for w_ in self.writes:
                    w_.result()
        finally:
            if self.own_ctx:
                self.ctx.close()

    def groups(self, jobs, frames, limit):
        """The plan: the jobs in descending frame order, cut into groups of at most `limit` frames."""
        return _batches(sorted(jobs, key=lambda i: -frames[i]), frames, limit)

    def batch(self, params=None, **lengths):
        """`with stage.batch(f0_lengths=...) as b`: a WorldBatch that is closed when the block is left, also by an
        exception.  Without params the batch only carries lengths (48 kHz, 5 ms: no stage of such a driver reads them)."""
        b = W.WorldBatch(self.ctx, params or W.default_params(48000, 5.0), **lengths)
        self.frames += int(b.total_frames)
        return contextlib.closing(b)

    def batches(self, jobs, frames, limit, params=None):
        """(group, stage.batch over the group's frame counts) along the plan."""
        for group in self.groups(jobs, frames, limit):
            yield group, self.batch(params, f0_lengths=[frames[i] for i in group])

    def load(self, paths, cols=None, want=None):
        """The float32 files `paths`, read by the pool as rows of `cols`, as one device tensor.  want: per path (frames,
        the file that says so), checked."""
        parts = list(self.pool.map(lambda p: _f32(p, cols), paths))
        for p, a, (n, first) in zip(paths, parts, want or ()):
            if len(a) != n:
                raise ValueError("%s has %d frames, %s has %d" % (p, len(a), first, n))
        return _upload(np.concatenate(parts))

    def submit(self, fn, *args):
        self.writes.append(self.pool.submit(fn, *args))

    def put(self, b, host, paths, head=None):
        """Utterance k's rows of the host slab to paths[k] (None: not written), one pool job each, beside the next
        batch; head(rows): bytes in front of them (an HTK header)."""
        for path, rows in _row_slices(b, host, paths):
            self.submit(_put, path, rows, head(len(rows)) if head else None)

    def put_native(self, b, slabs, threads):
        """slabs: [(host slab, paths)] as put takes them, all files in ONE native call (WorldMi355WriteFiles: plain
        threads, no interpreter lock) beside the next batch; the slabs live on in the job's arguments."""
        self.submit(W.write_files, [item for host, paths in slabs for item in _row_slices(b, host, paths)], threads)


def wav_header(path):
    """(sample count, sampling rate) from the header alone: what the partition needs (no samples are decoded)."""
    with wave.open(str(path), "rb") as w:
        return w.getnframes(), w.getframerate()


def outputs_complete(job, n_frames, fs, spec_dim=0, ap_dim=24):
    """True when the three feature files of `job` = (wav, f0_out, sp_out, ap_out) exist with exactly the sizes the
    analysis of this wav writes (float32: n_frames, n_frames x width, n_frames x width; width = CheapTrick's bins, or
    spec_dim / ap_dim in the recipe's coded form, analysis.cpp:292-390).  The test behind `resume`: a run that was cut
    short left its last files missing or short (the native writer creates, fills and closes file after file)."""
    bins = capi.cheaptrick_fft_size(fs) // 2 + 1
    want = (4 * n_frames, 4 * n_frames * (spec_dim if spec_dim else bins), 4 * n_frames * (ap_dim if spec_dim else bins))
    return all(_size_is(p, w) for p, w in zip(job[1:4], want))


def analysis_params(fs, frame_period, f0_floor=71.0, f0_ceil=800.0):
    """The analysis parameters of the recipe: the CLI's, with the f0 estimator's search range.  CheapTrick keeps the
    size the CLI gives it (GetFFTSizeForCheapTrick at its own 71 Hz, analysis.cpp:157-179): the files' row widths do not
    move with the search range."""
    if (float(f0_floor), float(f0_ceil)) == (71.0, 800.0):
        return W.default_params(fs, frame_period)
    if not 0.0 < f0_floor < f0_ceil:
        raise ValueError("f0 range %g - %g Hz" % (f0_floor, f0_ceil))
    return W.default_params(fs, frame_period, f0_floor=float(f0_floor), f0_ceil=float(f0_ceil),
                            fft_size=capi.cheaptrick_fft_size(fs))


def analysis_plan(order, frames, samples, max_batch_frames, params=None, f0_estimator="dio",
                  harvest_batch_bytes=None):
    """The batches of one sampling rate's utterances `order` (indices into frames and samples), in descending frame order
    as every driver's plan (_Stage.groups): closed at max_batch_frames, and with Harvest also at harvest_batch_bytes (sweep.HARVEST_BATCH_BYTES) of its workspace,
    whichever comes first; one utterance over a cap is a batch of its own.  Sample counts and parameters alone decide it."""
    from . import sweep
    W.f0_estimator_code(f0_estimator)
    fits = None
    if f0_estimator == "harvest":
        fits = sweep.harvest_fits(params, samples, sweep.HARVEST_BATCH_BYTES if harvest_batch_bytes is None
                                  else harvest_batch_bytes)
    return list(_batches(sorted(order, key=lambda i: -frames[i]), frames, max_batch_frames, fits))


def analysis_files(jobs, frame_period=5.0, fft_size=0, spec_dim=0, ap_dim=24, ctx=None,
                   max_batch_frames=MAX_BATCH_FRAMES, io_threads=8, gather=False, resume=False,
                   f0_estimator="dio", refine=True, f0_floor=71.0, f0_ceil=800.0, harvest_batch_bytes=None):
    """jobs: [(wav, f0_out, sp_out, ap_out)].  Writes what `analysis wav f0 sp ap frame_period fft_size
    [spec_dim [ap_dim]]` writes for every job; returns the number of frames analysed by this rank.

    f0_estimator "harvest": Harvest -> [StoneMask, with refine ->] CheapTrick -> D4C, the composition of the reference's
    functions that its CLI never made, in the same files; f0_floor / f0_ceil: the estimator's search range (analysis_params).
    With Harvest a batch also closes at harvest_batch_bytes of its workspace (None: sweep.HARVEST_BATCH_BYTES; analysis_plan).

    Every rank reads the wav HEADERS of the whole list (the partition needs the frame counts), but decodes only the
    utterances of its own shard, one batch at a time.  gather=False: every rank writes the files of its shard.
    gather=True (BASELINE.json configs[3]): the float32 slabs go to rank 0 (sweep.ShardedSweep), which writes all files.
    resume=True (every rank writes its shard only): a rank skips the jobs of ITS shard whose outputs are complete
    (outputs_complete) -- the partition is made on the whole list first, so ranks that start at different times agree on
    it whatever is on disk; the reference's recipe re-runs every utterance (data/Makefile.in:206-216)."""
    import torch  # noqa: F401 -- ahead of capi below, the first call into the library: where libworld_mi355.so is
    #                            loaded before torch, a fresh process's torch finds no GPU (`recipe.py analysis` did)
    jobs = list(jobs)
    if gather and resume:
        raise ValueError("resume goes with every rank writing its own shard (gather=False)")
    W.f0_estimator_code(f0_estimator)
    with ThreadPoolExecutor(io_threads) as pool:
        heads = list(pool.map(lambda j: wav_header(j[0]), jobs))
    frames = [sharding.frame_count(n, fs, frame_period) for n, fs in heads]
    for fs in sorted({h[1] for h in heads}):
        own_size = capi.cheaptrick_fft_size(fs)                    # GetFFTSizeForCheapTrick at the 71 Hz floor
        if fft_size not in (0, own_size):
            # analysis.cpp:157-179 sizes the rows by argv[6] but CheapTrick still runs at its own default
            # size for fs: any other value makes the reference write past or short of its rows
            raise ValueError("fft_size %d is not CheapTrick's size for %d Hz (%d)" % (fft_size, fs, own_size))
    with _Stage(ctx, io_threads) as stage:
        if gather:
            return _analysis_gathered(jobs, heads, frame_period, spec_dim, ap_dim, stage.ctx, max_batch_frames, io_threads,
                                      f0_estimator, refine, f0_floor, f0_ceil, harvest_batch_bytes)
        mine = _my_share(frames)
        if resume:
            mine = [i for i in mine if not outputs_complete(jobs[i], frames[i], heads[i][1], spec_dim, ap_dim)]
        for fs in sorted({heads[i][1] for i in mine}):
            params = analysis_params(fs, frame_period, f0_floor, f0_ceil)
            for group in analysis_plan([i for i in mine if heads[i][1] == fs], frames, [h[0] for h in heads],
                                       max_batch_frames, params, f0_estimator, harvest_batch_bytes):
                xs = [x for x, _ in stage.pool.map(lambda i: read_wav(jobs[i][0]), group)]   # this batch only, dropped after it
                with stage.batch(params, x_lengths=[len(x) for x in xs], f0_estimator=f0_estimator, refine=refine) as b:
                    x = _upload(np.concatenate(xs), pinned=True)
                    del xs
                    t, f0, sp, ap = b.analyze(x)
                    if spec_dim:
                        f0o, spo, apo = b.recipe_features(f0, sp, ap, spec_dim, ap_dim)     # analysis.cpp:292-366
                    else:
                        f0o, spo, apo = f0.float(), sp.float(), ap.float()                  # :360-390
                    stage.put_native(b, [(v.cpu().numpy(), [jobs[i][col] for i in group])
                                         for col, v in enumerate((f0o, spo, apo), 1)], io_threads)
    return stage.frames


def _rank_world():
    rank, world = 0, 1
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except ImportError:
        pass
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    return rank, world


def _analysis_gathered(jobs, heads, frame_period, spec_dim, ap_dim, ctx, max_batch_frames, io_threads,
                       f0_estimator="dio", refine=True, f0_floor=71.0, f0_ceil=800.0, harvest_batch_bytes=None):
    """configs[3]'s flow for a file list: shard, analyse, gather-v to rank 0, rank 0 writes (needs an initialised
    process group when there is more than one rank)."""
    import torch.distributed as dist
    from . import sweep
    rank, world = _rank_world()
    if world > 1 and not dist.is_initialized():
        raise RuntimeError("gather=True with WORLD_SIZE > 1 needs torch.distributed to be initialised")
    backend = dist.get_backend() if world > 1 else "nccl"
    done = 0
    for fs in sorted({h[1] for h in heads}):
        sel = [i for i, h in enumerate(heads) if h[1] == fs]
        sw = sweep.ShardedSweep(ctx, fs, frame_period, [heads[i][0] for i in sel], rank, world, spec_dim, ap_dim,
                                max_batch_frames, backend, f0_estimator=f0_estimator, refine=refine, f0_floor=f0_floor,
                                f0_ceil=f0_ceil, harvest_batch_bytes=sweep.HARVEST_BATCH_BYTES if harvest_batch_bytes is None
                                else harvest_batch_bytes)
        sw.load(lambda k: read_wav(jobs[sel[k]][0])[0], io_threads)
        sw.run(sweep.file_sink([jobs[i][1:4] for i in sel]) if rank == 0 else None, io_threads)
        done += sw.my_frames
        sw.close()
    return done


def synth_files(jobs, frame_period, fft_size, fs, spec_dim=0, ap_dim=24, ctx=None,
                max_batch_frames=MAX_BATCH_FRAMES, io_threads=8):
    """jobs: [(f0_in, sp_in, ap_in, wav_out)].  Writes what `synth f0 sp ap wav frame_period fft_size fs
    [spec_dim [ap_dim]]` writes.  In the coded form the ap bins beyond the coding order, which the reference
    leaves uninitialised (synth.cpp:240-245), are 0."""
    jobs = list(jobs)
    w = fft_size // 2 + 1
    cols = (None, spec_dim, ap_dim) if spec_dim else (None, w, w)
    frames = [os.path.getsize(j[0]) // 4 for j in jobs]                                     # synth.cpp:151-158
    mine = _my_share(frames)
    with _Stage(ctx, io_threads) as stage:
        params = W.default_params(fs, frame_period, fft_size=fft_size)
        for group in stage.groups(mine, frames, max_batch_frames):
            T = [frames[i] for i in group]
            ylen = [int((t - 1) * frame_period / 1000.0 * fs) + 1 for t in T]              # synth.cpp:259
            with stage.batch(params, f0_lengths=T, y_lengths=ylen) as b:
                f0, sp, ap = (stage.load([jobs[i][c] for i in group], cols[c]) for c in range(3))
                if spec_dim:
                    f0, sp, ap = b.recipe_decode(f0, sp, ap)                                # synth.cpp:168-256
                else:
                    f0, sp, ap = f0.double(), sp.double(), ap.double()
                y = b.synthesize(f0, sp, ap).cpu().numpy()
                yo = b.out_offsets
                for k, i in enumerate(group):
                    stage.submit(write_wav, jobs[i][3], y[yo[k]:yo[k + 1]], fs)
    return stage.frames


# ---- voice modification (test/test.cpp: analysis, ParameterModification :201-238, synthesis) ------------------------
MODIFY_D4C_THRESHOLD = 0.85           # InitializeD4COption's, which test.cpp:180-199 leaves as it is (analysis.cpp sets 0)


def read_modify_list(path, f0_scale=None, formant_ratio=None):
    """Lines `in.wav out.wav [f0_scale [formant_ratio]]`, test.cpp's argument order, as jobs (in, out, f0_scale,
    formant_ratio): a value the line leaves out is the argument's, and None -- "not done" -- without one."""
    jobs = []
    with open(path) as f:
        for ln in f:
            w = ln.split()
            if not w or ln.startswith("#"):
                continue
            if not 2 <= len(w) <= 4:
                raise ValueError("a line is `in.wav out.wav [f0_scale [formant_ratio]]`: %r" % ln.strip())
            try:
                given = [float(v) for v in w[2:]]
            except ValueError:
                raise ValueError("a factor is a number: %r" % ln.strip()) from None
            jobs.append((w[0], w[1], given[0] if len(given) > 0 else f0_scale, given[1] if len(given) > 1 else formant_ratio))
    return jobs


def modify_params(fs, frame_period=5.0, f0_floor=71.0, f0_ceil=800.0, d4c_threshold=MODIFY_D4C_THRESHOLD):
    """test.cpp's analysis settings: the CLI's (analysis_params) but for D4C's threshold."""
    p = analysis_params(fs, frame_period, f0_floor, f0_ceil)
    p.d4c_threshold = float(d4c_threshold)
    return p


def modify_samples(n_samples, fs, frame_period):
    """Samples of the wav made from one of n_samples: the batch's own y_length of its frame count (test.cpp:329-330)."""
    return int((sharding.frame_count(n_samples, fs, frame_period) - 1) * frame_period / 1000.0 * fs) + 1


def _put_wav16(path, pcm, fs):
    n = len(pcm)
    head = b"RIFF" + struct.pack("<I", 36 + n * 2) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, fs, fs * 2, 2, 16)
    _put(path, pcm, head + b"data" + struct.pack("<I", n * 2))


def _read_pcm16(path):
    with wave.open(str(path), "rb") as w:
        if w.getsampwidth() != 2:
            raise ValueError("%s: modify takes 16-bit samples, the file has %d-bit ones" % (path, 8 * w.getsampwidth()))
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


def modify_files(jobs, frame_period=5.0, f0_estimator="dio", f0_floor=71.0, f0_ceil=800.0,
                 d4c_threshold=MODIFY_D4C_THRESHOLD, ctx=None, max_batch_frames=MAX_BATCH_FRAMES, io_threads=8,
                 resume=False):
    """jobs: [(wav_in, wav_out, f0_scale, formant_ratio)], a factor of None meaning "not done" (read_modify_list).
    Writes what `test wav_in wav_out f0_scale formant_ratio` writes, with the f0 estimator named here in front:
    samples_from_pcm16, modify.convert (analyze, modify_features, synthesize), samples_to_pcm16, all on the device.
    A batch holds utterances of one sampling rate that give the same parts (a factor array covers a whole batch);
    rank-sharded by frame count; with resume a job whose wav_out has exactly the size of its result is skipped.
    Every factor is checked before a context is opened (ValueError).  Returns the frames converted by this rank."""
    import torch  # noqa: F401 -- ahead of the first call into the library (analysis_files says why)
    from . import modify as M
    jobs = [tuple(j) for j in jobs]
    if any(len(j) != 4 for j in jobs):
        raise ValueError("modify_files: a job is (wav_in, wav_out, f0_scale, formant_ratio)")
    W.f0_estimator_code(f0_estimator)
    with ThreadPoolExecutor(io_threads) as pool:
        heads = list(pool.map(lambda j: wav_header(j[0]), jobs))
    for j, (_, fs) in zip(jobs, heads):
        M.factor_array(j[0], "f0_scale", j[2], 1)
        M.factor_array(j[0], "formant_ratio", j[3], 1, capi.cheaptrick_fft_size(fs))
    frames = [sharding.frame_count(n, fs, frame_period) for n, fs in heads]
    mine = _my_jobs(frames, lambda i: not (resume and _size_is(jobs[i][1], 44 + 2 * modify_samples(heads[i][0], heads[i][1],
                                                                                                   frame_period))))
    if not mine:
        return 0
    kind = lambda i: (heads[i][1], jobs[i][2] is not None, jobs[i][3] is not None)
    with _Stage(ctx, io_threads) as stage:
        for fs, do_f0, do_sp in sorted({kind(i) for i in mine}):
            params = modify_params(fs, frame_period, f0_floor, f0_ceil, d4c_threshold)
            for group in analysis_plan([i for i in mine if kind(i) == (fs, do_f0, do_sp)], frames, [h[0] for h in heads],
                                       max_batch_frames, params, f0_estimator):
                pcm = list(stage.pool.map(lambda i: _read_pcm16(jobs[i][0]), group))
                with stage.batch(params, x_lengths=[len(a) for a in pcm], f0_estimator=f0_estimator) as b:
                    x = b.samples_from_pcm16(_upload(np.concatenate(pcm), pinned=True))
                    del pcm
                    y = M.convert(b, x, [jobs[i][2] for i in group] if do_f0 else None,
                                  [jobs[i][3] for i in group] if do_sp else None)
                    out = b.samples_to_pcm16(y).cpu().numpy()
                    yo = b.out_offsets
                    for k, i in enumerate(group):
                        stage.submit(_put_wav16, jobs[i][1], out[yo[k]:yo[k + 1]], int(fs))
    return stage.frames


def read_window(path):
    """data/win/NAME.winK: one line, the number of coefficients then the coefficients (window.pl:70-75)."""
    with open(path) as f:
        tok = f.readline().split()
    n = int(tok[0])
    return [float(v) for v in tok[1:1 + n]]


def _windows(ws):
    """A stream's windows as coefficient lists: each a window file (read_window) or the coefficients themselves."""
    return [read_window(w) if isinstance(w, (str, os.PathLike)) else [float(v) for v in w] for w in ws]


def _streams_arg(streams):
    return [(int(d), _windows(ws), bool(m)) for d, ws, m in streams]


def cmp_files(jobs, streams, sampling_rate, frame_shift, htk_type=9, ctx=None, max_batch_frames=MAX_BATCH_FRAMES,
              io_threads=8):
    """The recipe's `cmp` stage (data/Makefile.in:244-323): window.pl on every stream, the SPTK merge chain, and
    addhtkheader.pl, for a whole list.

    jobs:    [(stream_file_0, ..., stream_file_k, cmp_out)] -- float32 files [T][dim_s] in the order the recipe
             merges them (mgc, lf0, bap, vib); the four must have the same T
    streams: [(dim_s, [window files or coefficient lists])] per stream
    sampling_rate, frame_shift: addhtkheader.pl's SAMPFREQ and FRAMESHIFT (samples)"""
    jobs = list(jobs)
    ns = len(streams)
    dims = [int(d) for d, _ in streams]
    wins = [_windows(ws) for _, ws in streams]
    cols = sum(d * len(w) for d, w in zip(dims, wins))
    frames = [os.path.getsize(j[0]) // (4 * dims[0]) for j in jobs]
    mine = _my_share(frames)
    head = lambda n: W.htk_header(n, sampling_rate, frame_shift, 4 * cols, htk_type)
    with _Stage(ctx, io_threads) as stage:
        for group, batch in stage.batches(mine, frames, max_batch_frames, W.default_params(sampling_rate, 5.0)):
            with batch as b:
                want = [(frames[i], jobs[i][0]) for i in group]
                dev = [(stage.load([jobs[i][s_] for i in group], dims[s_], want), wins[s_]) for s_ in range(ns)]
                stage.put(b, b.compose_cmp(dev).cpu().numpy(), [jobs[i][ns] for i in group], head)
    return stage.frames


# ---- parameter generation (scripts/Training.pl:2755-2810 gen_param) ------------------------------------------------
def ffo_layout(streams):
    """Columns of an `ffo` row (Training.pl:2759-2765, :2778-2787): per stream its voicing column, when it has one, in
    front of its static and dynamic means.  streams: [(dim, windows, msd)].  Returns ([(msd column or None, first mean
    column, mean columns)], row width)."""
    at, out = 0, []
    for dim, wins, msd in streams:
        mcol = at if msd else None
        at += 1 if msd else 0
        out.append((mcol, at, int(dim) * len(wins)))
        at += int(dim) * len(wins)
    return out, at


def gen_param_complete(job, n_frames, streams):
    """True when every stream file of `job` = (ffo, out_0, ..., out_k) exists with the size generation writes
    (float32 [n_frames][dim_s]): the test behind `resume`, as outputs_complete is for analysis."""
    return all(_size_is(p, 4 * n_frames * int(d)) for p, (d, _, _) in zip(job[1:], streams))


def gen_param_files(jobs, streams, var_path, edge=0, unvoiced_value=-1.0e10, ctx=None,
                    max_batch_frames=MAX_BATCH_FRAMES, io_threads=8, resume=False):
    """`gen_param` (scripts/Training.pl:2755-2810) for a file list: SPTK `mlpg` on every stream of every utterance.

    jobs:     [(ffo_in, stream_out_0, ..., stream_out_k)] -- ffo_in: float32 rows of a model's output, per stream
              [voicing value, if the stream has one][static | delta | ...] (ffo_layout); stream_out_s: float32
              [T][dim_s], what :2797-2804 writes to $base.$type
    streams:  [(dim_s, [window files or coefficient lists, the static window first], msd)] in the row's order;
              a window file is data/win/NAME.winK: its leading size is dropped as `bcut -s 1` drops it (:2794)
    var_path: one float32 row in the ffo layout, the global variances (:2788-2791)
    A frame with voicing value below 0.5 (:2782) receives unvoiced_value in every dim of its stream (:2783, :2800-2801).
    Rank-sharded by frame count; with resume, utterances whose stream files are complete are skipped."""
    return _gen_param(jobs, streams, var_path, ctx, max_batch_frames, io_threads, resume,
                      lambda b, group, args: b.parameter_generation(args, edge=edge, unvoiced_value=unvoiced_value),
                      "the flagged columns are zeros")


def _gen_param(jobs, streams, var_path, ctx, max_batch_frames, io_threads, resume, generate, flagged_means):
    """gen_param_files and gen_param_gv_files: the job list, the plan and the stream files are the same;
    generate(batch, group, parameter_generation's streams) -> (outs, status) is the call in the middle."""
    jobs = list(jobs)
    streams = _streams_arg(streams)
    layout, width = ffo_layout(streams)
    var = np.fromfile(var_path, dtype=np.float32)
    if var.size != width:
        raise ValueError("%s has %d values, an ffo row has %d" % (var_path, var.size, width))
    frames = [_rows_in(j, width, 1 + len(streams), "%d output paths" % len(streams)) for j in jobs]
    mine = _my_jobs(frames, lambda i: not (resume and gen_param_complete(jobs[i], frames[i], streams)))
    with _Stage(ctx, io_threads) as stage:
        dvar = _upload(var)
        for group, batch in stage.batches(mine, frames, max_batch_frames):
            with batch as b:
                rows = stage.load([jobs[i][0] for i in group], width)
                args = [(rows[:, c0:c0 + n], dvar[c0:c0 + n], wins, None if mcol is None else rows[:, mcol])
                        for (mcol, c0, n), (_, wins, _) in zip(layout, streams)]
                outs, status = generate(b, [jobs[i] for i in group], args)
                for k in np.nonzero(status.cpu().numpy())[0]:
                    print("warning: %s: status %d, %s" % (jobs[group[k]][0], int(status[k]), flagged_means),
                          file=sys.stderr)
                for s_, o in enumerate(outs):
                    stage.put(b, o.cpu().numpy(), [jobs[i][1 + s_] for i in group])
    return stage.frames


# ---- parameter generation considering global variance (HMGenS with USEHMMGV = 1; scripts/Training.pl:1892-1903) --------
GV_OPTIONS = ("max_iter", "epsilon", "step_init", "step_inc", "step_dec", "hmm_weight", "gv_weight", "scale")


def gv_pdf_files(cmp_paths, out_dir):
    """The GV pdf of a corpus from the one-vector HTK files that gv_data_files writes (12 bytes of header, then one
    float32 row over the static columns of all streams): out_dir/gv.mean and out_dir/gv.var, the mean and the variance
    (dividing by n, as stats_files does) of every column over the files, float32.  Host only; in double, two passes.
    Returns the number of files read."""
    rows = [np.fromfile(str(p), dtype=np.float32, offset=12).astype(np.float64) for p in cmp_paths]
    if not rows:
        raise ValueError("gv_pdf_files: no file")
    for p, r in zip(cmp_paths, rows):
        if r.size != rows[0].size or r.size == 0:
            raise ValueError("%s holds %d values, %s holds %d" % (p, r.size, cmp_paths[0], rows[0].size))
    x = np.stack(rows)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    os.makedirs(str(out_dir), exist_ok=True)
    mean.astype(np.float32).tofile(os.path.join(str(out_dir), "gv.mean"))
    var.astype(np.float32).tofile(os.path.join(str(out_dir), "gv.var"))
    return len(rows)


def gv_label_mask(lines, frame_shift_s, n_rows, silences=()):
    """uint8 [n_rows]: 1 on the rows mspf_label_rows keeps, 0 on the rest -- the frames of the segments named in
    `silences` (the recipe's NOSILGV) and whatever no label line covers."""
    mask = np.zeros(n_rows, dtype=np.uint8)
    mask[mspf_label_rows(lines, frame_shift_s, n_rows, silences)] = 1
    return mask


def gen_param_gv_files(jobs, streams, var_path, gv_mean_path, gv_var_path, label_dir=None, silences=(),
                       frame_shift_s=0.005, edge=0, unvoiced_value=-1.0e10, ctx=None, max_batch_frames=MAX_BATCH_FRAMES,
                       io_threads=8, resume=False, **options):
    """gen_param_files with parameter generation considering global variance in mlpg's place
    (WorldBatch.parameter_generation_gv): the same jobs, streams, var_path, files and resume rule.

    gv_mean_path, gv_var_path: gv.mean and gv.var of gv_pdf_files, float32 rows over the static columns of all streams
    label_dir, silences: with both, <label_dir>/<base of ffo_in>.lab says where the segments named in `silences` lie
              (frames of frame_shift_s seconds, the rows of mspf_label_rows); GV is switched off in their frames
    options:  max_iter, epsilon, step_init, step_inc, step_dec, hmm_weight, gv_weight, scale (GV_OPTIONS); the recipe's
              defaults where left out
    A status of 1 or 4 leaves the column as gen_param_files writes it; see parameter_generation_gv."""
    unknown = sorted(set(options) - set(GV_OPTIONS))
    if unknown:
        raise TypeError("gen_param_gv_files: unknown option %s" % ", ".join(unknown))
    specs = _streams_arg(streams)
    static = sum(int(d) for d, _, _ in specs)
    gv = [np.fromfile(str(p), dtype=np.float32) for p in (gv_mean_path, gv_var_path)]
    for p, a in zip((gv_mean_path, gv_var_path), gv):
        if a.size != static:
            raise ValueError("%s has %d values, the streams have %d static columns" % (p, a.size, static))
    silences = tuple(silences)
    dev = {}

    def generate(b, group, args):
        if not dev:
            at = np.concatenate([[0], np.cumsum([int(d) for d, _, _ in specs])])
            dev["mean"] = [_upload(gv[0][at[k]:at[k + 1]]) for k in range(len(specs))]
            dev["var"] = [_upload(gv[1][at[k]:at[k + 1]]) for k in range(len(specs))]
        mask = None
        if label_dir is not None and silences:
            parts = []
            for k, job in enumerate(group):
                lab = os.path.join(str(label_dir), os.path.splitext(os.path.basename(job[0]))[0] + ".lab")
                with open(lab) as f:
                    parts.append(gv_label_mask(f.readlines(), frame_shift_s, int(b.frame_offsets[k + 1] - b.frame_offsets[k]),
                                               silences))
            mask = _upload(np.concatenate(parts))
        return b.parameter_generation_gv(args, dev["mean"], dev["var"], gv_mask=mask, edge=edge,
                                         unvoiced_value=unvoiced_value, **options)

    return _gen_param(jobs, streams, var_path, ctx, max_batch_frames, io_threads, resume, generate,
                      "columns flagged 1 or 2 by mlpg are zeros, the others are mlpg's")


# ---- trajectory training's criterion and outputs (scripts/Training.pl:930-940, DNNDefine.trajectory_cost) --------------
def trajectory_rows(streams):
    """float32 values per row of what trajectory_files writes: per stream its voicing column, when it has one, then dim."""
    return sum(int(d) + (1 if m else 0) for d, _, m in streams)


def trajectory_files(jobs, streams, var_path, gv_path, msd_weight=1.0, gv_weight=1.0e-6, ctx=None,
                     max_batch_frames=MAX_BATCH_FRAMES, io_threads=8, resume=False):
    """What DNNSynthesis.py does with a model trained by trajectory training ($TRJGV), for a file list: the rows of
    DNNDefine.trajectory_cost's final_outputs and, where the targets are given, the cost of every utterance.

    jobs:     [(pred_ffo, obs_ffo or None, out or None)] -- pred_ffo: float32 rows of the model's output in the ffo
              layout; obs_ffo: the targets in the same layout (ffo_files writes them); out: float32 [T][sum_s (msd_s +
              dim_s)], per stream the predicted voicing column, when it has one, then the trajectory c
    streams:  [(dim_s, [window files or coefficient lists, the static window first], msd)] as gen_param_files takes them
    var_path: one float32 row in the ffo layout (ffo.var or the trained variances); gv_path: gv.var, one float32 row
              over the static columns of all streams in order
    With obs_ffo the rows and the cost come from WorldBatch.trajectory_cost; without it the trajectories are
    parameter_generation's (edge 0, no voicing mask) and no cost is evaluated.  Returns one entry per job: the cost
    trj + msd_weight msd + gv_weight gv, or None (no targets; skipped by resume; another rank's; a flagged utterance,
    which is reported on stderr and whose flagged columns are zeros).  Rank-sharded by frame count."""
    from . import training
    jobs = [tuple(j) for j in jobs]
    streams = _streams_arg(streams)
    layout, width = ffo_layout(streams)
    out_cols = trajectory_rows(streams)
    var = np.fromfile(var_path, dtype=np.float32)
    if var.size != width:
        raise ValueError("%s has %d values, an ffo row has %d" % (var_path, var.size, width))
    need_gv = any(j[1] is not None for j in jobs)
    if need_gv:
        gv = np.fromfile(gv_path, dtype=np.float32)
        if gv.size != sum(d for d, _, _ in streams):
            raise ValueError("%s has %d values, the streams have %d static columns" % (gv_path, gv.size, sum(d for d, _, _ in streams)))
    frames = []
    for j in jobs:
        frames.append(_rows_in(j, width, 3, "(pred, obs, out)"))
        if j[1] is not None and os.path.getsize(j[1]) != 4 * width * frames[-1]:
            raise ValueError("%s and %s differ in size" % (j[0], j[1]))
    mine = _my_jobs(frames, lambda i: not (resume and jobs[i][2] is not None
                                           and _size_is(jobs[i][2], 4 * frames[i] * out_cols)))
    costs = [None] * len(jobs)
    with _Stage(ctx, io_threads) as stage:
        dvar = _upload(var)
        dgv = _upload(gv) if need_gv else None
        for with_obs in (True, False):
            part = [i for i in mine if (jobs[i][1] is not None) == with_obs]
            for group, batch in stage.batches(part, frames, max_batch_frames):
                with batch as b:
                    load = lambda col: stage.load([jobs[i][col] for i in group], width)
                    pred = load(0)
                    if with_obs:
                        cost, c, _, _, status = b.trajectory_cost(training.stream_views(pred, load(1), streams), dvar, dgv,
                                                                  msd_weight, gv_weight, want_grad_pred=False,
                                                                  want_grad_var=False)
                        total = (cost[:, 0] + msd_weight * cost[:, 1] + gv_weight * cost[:, 2]).cpu().numpy()
                    else:
                        c, status = b.parameter_generation([(pred[:, c0:c0 + n], dvar[c0:c0 + n], wins, None)
                                                            for (_, c0, n), (_, wins, _) in zip(layout, streams)], edge=0)
                    status = status.cpu().numpy()
                    for k in np.nonzero(status)[0]:
                        print("warning: %s: status %d, the flagged columns are zeros" % (jobs[group[k]][0], int(status[k])),
                              file=sys.stderr)
                    stage.put(b, training.final_outputs(b, pred, c, streams).cpu().numpy(), [jobs[i][2] for i in group])
                    for k, i in enumerate(group):
                        if with_obs and status[k] == 0:
                            costs[i] = float(total[k])
    return costs


def read_forward_scp(path):
    """The scp of Training.pl:1691-1722 as DNNDataIO.get_filenames reads it: a line is `ffi` or `ffi ffo`."""
    jobs = []
    with open(path) as f:
        for ln in f:
            if not ln.strip():
                continue
            if " " not in ln.rstrip("\n").rstrip():
                jobs.append((ln.strip(), None))
            else:
                a, b_ = ln.split(" ", 1)
                jobs.append((a.strip(), b_.strip()))
    return jobs


def forward_files(jobs, model_path, out_dir, spkr=None, extension="ffo", ctx=None, max_batch_frames=MAX_BATCH_FRAMES,
                  io_threads=8, max_chunk_frames=0, report=print):
    """What DNNSynthesis.py does frame by frame (scripts/Training.pl:877, 906, 964, 993), for a file list: the model's
    outputs for every `.ffi`, the speaker's variance row beside them and, where the targets are paired, the cost.

    jobs:       [(ffi, ffo or None)] (read_forward_scp) -- ffi: float32 rows of the model's n_inputs; ffo: the targets
    model_path: the `.npz` training.AcousticModel.save writes
    spkr:       None: the last speaker, as the script (DNNSynthesis.py:139); or one index for every file
    Writes <out_dir>/<base>.<extension> (the means in the ffo layout: what gen_param_files and trajectory_files read)
    and <out_dir>/<base>.var (DNNSynthesis.py:202).  For every pair the cost is reported as `Evaluation: cost = %e (ffi)`:
    the script's line (DNNSynthesis.py:233), whose parenthesis holds the elapsed time, with the file's name there instead,
    since one run covers many files (as `trj-eval` does).
    Returns one entry per job: the cost, or None (no targets; another rank's; a flagged utterance, which is reported on
    stderr and whose rows are zeros).  Rank-sharded by frame count."""
    import torch
    from . import training
    jobs = [tuple(j) if not isinstance(j, (str, os.PathLike)) else (j, None) for j in jobs]
    model = training.AcousticModel.load(model_path)
    n_in, n_out = model.n_inputs, model.n_outputs
    s_id = model.n_spkrs - 1 if spkr is None else int(spkr)
    if not 0 <= s_id < model.n_spkrs:
        raise ValueError("speaker %d: the model has %d" % (s_id, model.n_spkrs))
    frames = []
    for j in jobs:
        frames.append(_rows_in(j, n_in, 2, "(ffi, ffo)"))
        if j[1] is not None and os.path.getsize(j[1]) != 4 * n_out * frames[-1]:
            raise ValueError("%s does not hold %d rows of %d float32, as %s asks" % (j[1], frames[-1], n_out, j[0]))
    mine = [i for i in _my_share(frames) if frames[i] > 0]
    bases = [os.path.join(str(out_dir), os.path.splitext(os.path.basename(j[0]))[0]) for j in jobs]
    costs = [None] * len(jobs)
    with _Stage(ctx, io_threads) as stage:
        model = model.cuda()
        var_row = model.variance.variances[s_id].detach().to(torch.float32).cpu().numpy()
        os.makedirs(str(out_dir), exist_ok=True)
        for with_obs in (True, False):
            part = [i for i in mine if (jobs[i][1] is not None) == with_obs]
            for group, batch in stage.batches(part, frames, max_batch_frames):
                with batch as b:
                    load = lambda col, w: stage.load([jobs[i][col] for i in group], w)
                    out, cost, status = model.infer(b, load(0, n_in), [s_id] * len(group),
                                                    load(1, n_out) if with_obs else None, max_chunk_frames)
                    host, status = out.cpu().numpy(), status.cpu().numpy()
                    cost = cost.cpu().numpy() if cost is not None else None
                    for k, i in enumerate(group):
                        if status[k]:
                            print("warning: %s: status %d, its rows are zeros" % (jobs[i][0], int(status[k])), file=sys.stderr)
                        elif with_obs:
                            costs[i] = float(cost[k])
                            report("    Evaluation: cost = %e (%s)" % (costs[i], jobs[i][0]))
                        stage.submit(var_row.tofile, bases[i] + ".var")
                    stage.put(b, host, [bases[i] + "." + extension if extension else bases[i] for i in group])
    return costs


# ---- the training loop: DNNTraining.py frame by frame, SD and SAT (scripts/Training.pl:850-870) ------------------------
OPTIMIZERS = ("sgd", "momentum", "adagrad", "adadelta", "adam", "rmsprop")     # DNNDefine.get_optimizer (DNNDefine.py:65-80)


def make_optimizer(model, name, learning_rate):
    """DNNDefine.training's three groups (DNNDefine.py:194-213): the si_ parameters at learning_rate, the sd_ parameters
    at learning_rate, the variances at 0.01 learning_rate -- as torch.optim's optimiser of that name with TF 1.x's
    default hyper-parameters (momentum 0.9; Adagrad's accumulator 0.1; Adadelta rho 0.95, eps 1e-8; Adam 0.9, 0.999,
    1e-8; RMSprop decay 0.9, eps 1e-10).  torch adds Adam's and RMSprop's eps outside the square root, TF inside it for
    RMSprop and to a rescaled root for Adam; and TF 1.x starts RMSprop's mean-square slot at ones, torch at zeros, so
    RMSprop's first steps are much larger here (the first about 1 / sqrt(0.1) times the rate, against about the gradient
    times the rate in TF).  These trajectories are not TF's; Tf1Optimizer's follow TF's rules."""
    import torch
    named = list(model.named_parameters())
    pick = lambda key: [p for k, p in named if k.split(".")[-1].startswith(key)]
    groups = [{"params": pick("si_"), "lr": learning_rate}, {"params": pick("sd_"), "lr": learning_rate},
              {"params": pick("variance"), "lr": 0.01 * learning_rate}]
    groups = [g for g in groups if g["params"]]
    name = name.lower()
    if name == "sgd":
        return torch.optim.SGD(groups, lr=learning_rate)
    if name == "momentum":
        return torch.optim.SGD(groups, lr=learning_rate, momentum=0.9)
    if name == "adagrad":
        return torch.optim.Adagrad(groups, lr=learning_rate, initial_accumulator_value=0.1, eps=0.0)
    if name == "adadelta":
        return torch.optim.Adadelta(groups, lr=learning_rate, rho=0.95, eps=1e-8)
    if name == "adam":
        return torch.optim.Adam(groups, lr=learning_rate, betas=(0.9, 0.999), eps=1e-8)
    if name == "rmsprop":
        return torch.optim.RMSprop(groups, lr=learning_rate, alpha=0.9, eps=1e-10)
    raise ValueError("an optimiser is one of %s" % (OPTIMIZERS,))


class Tf1Optimizer:
    """make_optimizer's three groups (by the same test on the parameter's name) under TF 1.x's own update rules -- the
    table in include/world_mi355.h, float32, every operation rounded on its own -- with the state tf.train.Saver keeps:
    the slots per parameter and Adam's two beta powers.  The rates are (learning_rate, learning_rate, 0.01 learning_rate)
    for the si_ parameters, the sd_ parameters and the variances; with adapt (DNNTraining.py's ADAPT mode, :297-303)
    (0, learning_rate, 0.01 learning_rate): at rate 0 the slots move and the parameter keeps its bits.

    ctx: the world.Context whose optimizer_step updates every tensor in one launch (the parameters are float32 cuda
    tensors); or None: the same sequence of operations in torch float32 on the CPU, for parameters on the CPU -- the
    loop's host path, as train_files(device="cpu") is.  step() reads every parameter's .grad and advances the powers."""

    def __init__(self, model, name, learning_rate, ctx, adapt=False):
        import torch
        name = name.lower()
        if name not in OPTIMIZERS:
            raise ValueError("an optimiser is one of %s" % (OPTIMIZERS,))
        self.name, self.rule, self.ctx = name, W.OPTIMIZER_RULES.index(name), ctx
        rate_of = (("si_", 0.0 if adapt else learning_rate), ("sd_", learning_rate), ("variance", 0.01 * learning_rate))
        self.names, self.params, self.rates = [], [], []
        for key, rate in rate_of:
            for k, p in model.named_parameters():
                if k.split(".")[-1].startswith(key):
                    self.names.append(k)
                    self.params.append(p)
                    self.rates.append(float(np.float32(rate)))
        for p in self.params:
            if p.dtype != torch.float32 or p.is_cuda != (ctx is not None) or not p.is_contiguous():
                raise ValueError("Tf1Optimizer: float32 contiguous parameters, on the GPU with a context and on the CPU without")
        self.slots = [[torch.full_like(p, v) for p in self.params] for v in W.OPTIMIZER_SLOT_INIT[self.rule]]
        # TF 1.x's defaults in float32, as WorldMi355DefaultOptimizerOption sets them
        f = np.float32
        self.momentum, self.rho = f(0.9), f(0.95 if name == "adadelta" else 0.9)
        self.beta1, self.beta2, self.epsilon = f(0.9), f(0.999), f(1e-10 if name == "rmsprop" else 1e-8)
        self.beta1_power, self.beta2_power = self.beta1, self.beta2

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def step(self):
        import torch
        grads = []
        for k, p in zip(self.names, self.params):
            if p.grad is None:
                raise RuntimeError("Tf1Optimizer.step: %s has no gradient" % k)
            grads.append(p.grad.to(torch.float32).contiguous())
        with torch.no_grad():
            if self.ctx is not None:
                o = W.default_optimizer_option(self.rule, beta1_power=float(self.beta1_power), beta2_power=float(self.beta2_power))
                self.ctx.optimizer_step(o, [p.data for p in self.params], grads, self.rates, *self.slots)
            else:
                for i, (p, g, r) in enumerate(zip(self.params, grads, self.rates)):
                    self._host_update(p, g, r, [s[i] for s in self.slots])
        self.beta1_power, self.beta2_power = self.beta1_power * self.beta1, self.beta2_power * self.beta2

    def _host_update(self, p, g, r, slots):
        """The table's operations one by one: torch's float32 CPU operations round each on its own, and no call here is
        a fused one (no addcmul, no alpha=)."""
        import torch
        f = np.float32
        c = lambda v: float(f(v))                     # a float32 value as the Python float torch casts back to it exactly
        one = f(1.0)
        if self.name == "sgd":
            p.copy_(p - g * c(r))
        elif self.name == "momentum":
            a, = slots
            a.copy_(a * c(self.momentum) + g)
            p.copy_(p - a * c(r))
        elif self.name == "adagrad":
            a, = slots
            a.copy_(a + g * g)
            p.copy_(p - (g * c(r)) / torch.sqrt(a))
        elif self.name == "adadelta":
            a, b = slots
            rho, eps = c(self.rho), c(self.epsilon)
            a.copy_(a * rho + (g * g) * c(one - self.rho))
            u = (torch.sqrt(b + eps) / torch.sqrt(a + eps)) * g
            p.copy_(p - u * c(r))
            b.copy_(b * rho + (u * u) * c(one - self.rho))
        elif self.name == "adam":
            m, v = slots
            alpha = f(f(r) * np.sqrt(one - self.beta2_power)) / (one - self.beta1_power)
            m.copy_(m + (g - m) * c(one - self.beta1))
            v.copy_(v + (g * g - v) * c(one - self.beta2))
            p.copy_(p - (m * c(alpha)) / (torch.sqrt(v) + c(self.epsilon)))
        else:
            s, = slots
            s.copy_(s + (g * g - s) * c(one - self.rho))
            p.copy_(p - (g * c(r)) / torch.sqrt(s + c(self.epsilon)))

    def state_arrays(self):
        """What AcousticModel.save(optimizer_state=...) writes: the rule's name, slot0/<parameter name> and
        slot1/<parameter name> as float32 arrays, and the two beta powers."""
        out = {"rule": np.array(self.name)}
        for j, slot in enumerate(self.slots):
            for k, t in zip(self.names, slot):
                out["slot%d/%s" % (j, k)] = t.detach().cpu().numpy().copy()
        out["beta1_power"] = np.array(self.beta1_power, dtype=np.float32)
        out["beta2_power"] = np.array(self.beta2_power, dtype=np.float32)
        return out

    def load_state_arrays(self, state):
        """Continue from state_arrays()' dictionary (AcousticModel.load leaves it in the module's optimizer_state)."""
        import torch
        if str(state.get("rule")) != self.name:
            raise ValueError("the state is of optimiser %s, not %s" % (state.get("rule"), self.name))
        with torch.no_grad():
            for j, slot in enumerate(self.slots):
                for k, t in zip(self.names, slot):
                    v = state.get("slot%d/%s" % (j, k))
                    if v is None or tuple(v.shape) != tuple(t.shape):
                        raise ValueError("the state holds no slot%d of %s of shape %s" % (j, k, tuple(t.shape)))
                    t.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)))
        self.beta1_power, self.beta2_power = np.float32(state["beta1_power"]), np.float32(state["beta2_power"])


def minibatches(frame_spkr, batch_size, n_steps, seed, start=0):
    """The frame-by-frame minibatches of steps start .. start + n_steps - 1: every epoch a permutation of the frames by
    numpy.random.default_rng(seed) (the epochs draw from one generator), cut into batch_size frames (an epoch's tail
    shorter than that is dropped, as the reader's queue leaves it).  Yields (rows, lengths, spkrs): the frames' indices
    grouped into one pseudo-utterance per speaker present, speakers ascending and the draw's order kept within one."""
    frame_spkr = np.asarray(frame_spkr)
    for rows in _draws(len(frame_spkr), batch_size, n_steps, seed, start, "frames"):
        rows = rows[np.argsort(frame_spkr[rows], kind="stable")]
        spkrs, lengths = np.unique(frame_spkr[rows], return_counts=True)
        yield rows, [int(v) for v in lengths], [int(v) for v in spkrs]


def utterance_minibatches(file_spkr, batch_size, n_steps, seed, start=0):
    """Trajectory training's minibatches: batch_size files of the same seeded permutations.  Yields (files, spkrs): the
    files' indices ordered by speaker (the draw's order kept within one) and the speaker of each."""
    file_spkr = np.asarray(file_spkr)
    for files in _draws(len(file_spkr), batch_size, n_steps, seed, start, "files"):
        files = files[np.argsort(file_spkr[files], kind="stable")]
        yield files, [int(v) for v in file_spkr[files]]


def _draws(n, batch_size, n_steps, seed, start, what):
    if batch_size < 1 or n < batch_size:
        raise ValueError("%d %s do not fill a minibatch of %d" % (n, what, batch_size))
    rng = np.random.default_rng(seed)
    done = 0
    while done < start + n_steps:
        perm = rng.permutation(n)
        for at in range(0, n - batch_size + 1, batch_size):
            if done == start + n_steps:
                return
            if done >= start:
                yield perm[at:at + batch_size]
            done += 1


def _train_cost(model, b, x, obs, lengths, spkrs, keep_prob, seed, step):
    """The minibatch's cost (a float64 scalar with autograd history): the mean over its frames of DNNDefine.cost, from
    the library's training pass (training.AcousticModel.train_outputs and training.FrameLoss) on the WorldBatch `b` of
    the pseudo-utterances, which must live until the cost's backward() has run."""
    import torch
    from . import training
    out = model.train_outputs(b, x, spkrs, keep_prob, seed, step)
    cost = training.FrameLoss.apply(b, out, model.variance.variances, obs, spkrs)
    w = torch.as_tensor(lengths, dtype=torch.float64, device=cost.device)
    return (cost * (w / w.sum())).sum()


def _train_cost_trajectory(model, b, parts, x, obs, spkrs, layout, gv_var, msd_weight, gv_weight, keep_prob, seed, step):
    """Trajectory training's cost of a minibatch of utterances ordered by speaker (DNNDefine.trajectory_cost: the mean
    over the utterances): one training forward on the WorldBatch `b` of all of them, then training.TrajectoryLoss per
    speaker present, with that speaker's variance row and GV variances, on parts = [(speaker, WorldBatch of its
    utterances, first row, end row)].  Every batch must live until the cost's backward() has run."""
    from . import training
    out = model.train_outputs(b, x, spkrs, keep_prob, seed, step)
    total = 0.0
    for s, sub, r0, r1 in parts:
        total = total + training.TrajectoryLoss.apply(sub, out[r0:r1], model.variance.variances[s], obs[r0:r1], gv_var[s],
                                                      layout, msd_weight, gv_weight).sum()
    return total / len(spkrs)


def _variance_rows(variance_dir, name, n_spkrs, width):
    """DNNTraining.py:116-139: <dir>/<name> in SD mode, <dir>/<speaker index>/<name> per speaker in SAT mode."""
    rows = [_f32(os.path.join(str(variance_dir), name) if n_spkrs == 1 else
                 os.path.join(str(variance_dir), str(s), name)).reshape(-1) for s in range(n_spkrs)]
    if any(r.shape != (width,) for r in rows):
        raise ValueError("%s: %s does not hold %d float32" % (variance_dir, name, width))
    return np.stack(rows)


def train_files(jobs, model_path, n_inputs, units, n_outputs, n_spkrs=1, variance_dir=None, hidden_activation="sigmoid",
                output_activation="linear", keep_prob=0.5, optimizer="adam", learning_rate=0.001, batch_size=256,
                n_epochs=100, n_steps=None, seed=0, log_interval=100, save_interval=0, restore=None, streams=None,
                msd_weight=1.0, gv_weight=1.0e-6, ctx=None, device="cuda", report=print, updates="torch", adapt=False):
    """What DNNTraining.py does in SD, SAT and ADAPT mode: trains the acoustic model on a file list and saves it.

    jobs:         [(ffi, ffo)] or [(ffi, ffo, speaker index)]: float32 rows of n_inputs and of n_outputs
    model_path:   the `.npz` to write (training.AcousticModel.save, with the step count): every save_interval steps
                  (0: never) and at the end
    units:        the hidden layers' widths; n_spkrs > 1 is SAT mode
    variance_dir: None (variances and GV variances 1), or DNNTraining.py -z: the directory of ffo.var and gv.var (SAT:
                  <dir>/<speaker index>/ffo.var and gv.var)
    streams:      None: frame by frame, DNNDefine.cost on minibatches of batch_size frames (minibatches); or DNNTraining.py
                  -w, trajectory training: [(dim, windows, msd)] in the row's order as trajectory_files takes it,
                  DNNDefine.trajectory_cost (training.TrajectoryLoss, with msd_weight and gv_weight) on minibatches of
                  batch_size utterances (utterance_minibatches).  The GV variances stay at gv.var: the library returns no
                  gradient with respect to them, and the `.npz` does not hold them
    restore:      None, or the `.npz` to continue from: the steps, the minibatch draws and the dropout offsets go on from
                  its step count.  With updates="tf1" the optimiser's own state (the slots, Adam's beta powers) goes on
                  from the file's too, as with tf.train.Saver: a continued run is the run it continues, bit for bit.  A
                  file without the state of this optimiser is reported in one line, and the state begins anew; with
                  updates="torch" it always begins anew
    updates:      "torch": one step of make_optimizer's optimiser (torch.optim's rules).  "tf1": one step of Tf1Optimizer
                  (TF 1.x's rules; on the GPU one launch of the library's kernel), whose state every save writes
    adapt:        DNNTraining.py's ADAPT mode (:102-107, 297-303, 323-328): needs `restore` with a SAT model of at least
                  two speakers.  Before the first step every hidden layer's sd_weights[-1] becomes the float32 mean of the
                  other speakers' rows; the si_ parameters then train at rate 0, the sd_ parameters at learning_rate, the
                  variances at 0.01 learning_rate.  The jobs are the new (last) speaker's
    A step runs the library's training forward and backward with dropout (seed, offset = the step number) and one step of
    the optimiser.  n_steps: None for n_epochs * frames // batch_size, in trajectory mode n_epochs * files //
    batch_size (DNNTraining.py:180-187).  Every log_interval steps `Step %7d: cost = %e` is reported (DNNTraining.py:369).
    Returns the reported (step, cost) pairs.  The whole corpus is held on the device."""
    import torch
    from . import training
    jobs = [tuple(j) + (0,) * (3 - len(j)) for j in jobs]
    if updates not in ("torch", "tf1"):
        raise ValueError("updates is \"torch\" or \"tf1\"")
    if adapt and (restore is None or n_spkrs < 2):
        raise ValueError("adapt continues a SAT model of at least two speakers: give restore")
    frames = []
    for ffi, ffo, s in jobs:
        size = os.path.getsize(ffi)
        if size % (4 * n_inputs) or os.path.getsize(ffo) != size // (4 * n_inputs) * 4 * n_outputs:
            raise ValueError("%s, %s: not as many rows of %d and %d float32" % (ffi, ffo, n_inputs, n_outputs))
        if not 0 <= int(s) < n_spkrs:
            raise ValueError("%s: speaker %d of %d" % (ffi, s, n_spkrs))
        frames.append(size // (4 * n_inputs))
    layout = n_static = None
    if streams is not None:
        layout = _streams_arg(streams)
        n_static = sum(d for d, _, _ in layout)
        if ffo_layout(layout)[1] != n_outputs:
            raise ValueError("the streams make rows of %d columns, not %d" % (ffo_layout(layout)[1], n_outputs))
    if n_steps is None:
        n_steps = n_epochs * (sum(frames) if layout is None else len(jobs)) // batch_size
    torch.manual_seed(seed)                                        # the initialisation's draws
    start = 0
    if restore is not None:
        model = training.AcousticModel.load(restore)
        if (model.n_inputs, model.units, model.n_outputs, model.n_spkrs) != (n_inputs, [int(n) for n in units], n_outputs, n_spkrs):
            raise ValueError("%s holds another net" % restore)
        start = model.step
        if adapt:
            if not model.sat:
                raise ValueError("%s is no SAT model: nothing to adapt" % restore)
            for i in range(len(model.units)):                          # DNNTraining.py:323-328
                sd = model.hidden(i).sd_weights.detach().numpy()       # (the parameter's own memory)
                sd[-1] = np.mean(sd[:-1], 0)
    else:
        model = training.AcousticModel(n_inputs, units, n_outputs, n_spkrs, hidden_activation, output_activation)
        if variance_dir is not None:                               # DNNTraining.py:116-127
            with torch.no_grad():
                model.variance.variances.copy_(torch.from_numpy(_variance_rows(variance_dir, "ffo.var", n_spkrs, n_outputs)))
    gv_var = None
    if layout is not None:                                         # DNNTraining.py:129-139
        gv_var = torch.from_numpy(_variance_rows(variance_dir, "gv.var", n_spkrs, n_static) if variance_dir is not None
                                  else np.ones((n_spkrs, n_static), dtype=np.float32)).to(device)
    model = model.to(device)
    own_ctx = ctx is None and device != "cpu"
    if own_ctx:
        ctx = _own_context()
    try:
        x = torch.from_numpy(np.concatenate([_f32(j[0], n_inputs) for j in jobs])).to(device)
        obs = torch.from_numpy(np.concatenate([_f32(j[1], n_outputs) for j in jobs])).to(device)
        file_spkr = [int(j[2]) for j in jobs]
        f_off = np.concatenate([[0], np.cumsum(frames)])
        if updates == "tf1":
            opt = Tf1Optimizer(model, optimizer, learning_rate, ctx, adapt)
            state = model.optimizer_state if restore is not None else None
            if state is not None and str(state.get("rule")) == opt.name:
                opt.load_state_arrays(state)
            elif restore is not None:
                report("%s holds no state of optimiser %s: its state begins anew" % (restore, opt.name))
        else:
            opt = make_optimizer(model, optimizer, learning_rate)
            if adapt:
                si = {id(p) for k, p in model.named_parameters() if k.split(".")[-1].startswith("si_")}
                for g in opt.param_groups:
                    if g["params"] and id(g["params"][0]) in si:
                        g["lr"] = 0.0
        state_of = (lambda: opt.state_arrays()) if updates == "tf1" else (lambda: None)
        batch = (lambda lengths: W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=lengths)) if ctx is not None \
            else (lambda lengths: None)
        draws = minibatches(np.repeat(file_spkr, frames), batch_size, n_steps, seed, start) if layout is None \
            else utterance_minibatches(file_spkr, batch_size, n_steps, seed, start)
        log = []
        for step, draw in enumerate(draws, start):
            opt.zero_grad(set_to_none=True)
            live = []
            try:
                if layout is None:
                    rows, lengths, spkrs = draw
                    idx = torch.from_numpy(rows).to(device)
                    live.append(batch(lengths))
                    cost = _train_cost(model, live[0], x[idx], obs[idx], lengths, spkrs, keep_prob, seed, step)
                else:
                    files, spkrs = draw
                    lengths = [frames[i] for i in files]
                    idx = torch.from_numpy(np.concatenate([np.arange(f_off[i], f_off[i + 1]) for i in files])).to(device)
                    live.append(batch(lengths))
                    parts, off = [], np.concatenate([[0], np.cumsum(lengths)])
                    for s in sorted(set(spkrs)):
                        k0, k1 = spkrs.index(s), len(spkrs) - spkrs[::-1].index(s)
                        live.append(batch(lengths[k0:k1]))
                        parts.append((s, live[-1], int(off[k0]), int(off[k1])))
                    cost = _train_cost_trajectory(model, live[0], parts, x[idx], obs[idx], spkrs, layout, gv_var, msd_weight,
                                                  gv_weight, keep_prob, seed, step)
                cost.backward()
            finally:
                for b in live:
                    if b is not None:
                        b.close()
            opt.step()
            if log_interval > 0 and ((step - start) % log_interval == 0 or step == start + n_steps - 1):
                log.append((step, float(cost.detach())))
                report("Step %7d: cost = %e" % log[-1])
            if save_interval > 0 and (step + 1 - start) % save_interval == 0 and step + 1 < start + n_steps:
                model.save(model_path, step + 1, state_of())
        model.save(model_path, start + n_steps, state_of())
    finally:
        if own_ctx:
            ctx.close()
    return log


# ---- training targets, their variances and the GV data (data/Makefile.in:325-459, Training.pl:1402-1491) -------------
def _stream_frames(jobs, dims, n_paths, what):
    """Frames per job from the first stream file's size; every stream file of a job must hold as many rows."""
    frames = []
    for j in jobs:
        frames.append(_rows_in(j, dims[0], n_paths, what))
        for path, dim in zip(j[1:len(dims)], dims[1:]):
            other = os.path.getsize(path)
            if other != 4 * dim * frames[-1]:
                raise ValueError("%s has %g frames, %s has %d" % (path, other / (4.0 * dim), j[0], frames[-1]))
    return frames


def ffo_files(jobs, streams, unvoiced_value=-1.0e10, ctx=None, max_batch_frames=MAX_BATCH_FRAMES, io_threads=8,
              resume=False):
    """The recipe's `ffo` stage (data/Makefile.in:325-412) for a file list: the frame-by-frame training targets.

    jobs:    [(stream_file_0, ..., stream_file_k, ffo_out)] -- float32 files [T][dim_s] in the row's order (mgc, lf0,
             bap, vib); ffo_out: float32 [T][row width], the row of ffo_layout (no header)
    streams: [(dim_s, [window files or coefficient lists], msd)], the triple gen_param_files takes
    A stream with msd is interpolated across the frames that hold unvoiced_value (interpolate.pl), flagged (`sopr
    -magic -1.0E+10 -m 0 -a 1 -MAGIC 0`, from its column 0) and windowed; the others are windowed (:373-408).  An
    utterance whose msd stream has a column without a valid value is reported on stderr and its ffo is not written:
    interpolate.pl dies there and the Makefile's `-s` tests skip the utterance.  Frame counts must agree across an
    utterance's files.  Rank-sharded by frame count; with resume, utterances whose ffo file is complete are skipped.
    Returns the frames composed."""
    jobs = list(jobs)
    streams = _streams_arg(streams)
    ns = len(streams)
    width = ffo_layout(streams)[1]
    frames = _stream_frames(jobs, [d for d, _, _ in streams], ns + 1, "%d stream files and one output path" % ns)
    mine = _my_jobs(frames, lambda i: frames[i] > 0 and not (resume and _size_is(jobs[i][ns], 4 * width * frames[i])))
    if not mine:
        return 0
    with _Stage(ctx, io_threads) as stage:
        for group, batch in stage.batches(mine, frames, max_batch_frames):
            with batch as b:
                dev, bad = [], np.zeros(len(group), dtype=np.int32)
                for s_, (dim, wins, msd) in enumerate(streams):
                    x, voiced = stage.load([jobs[i][s_] for i in group], dim), None
                    if msd:
                        x, voiced, status = b.interpolate_gaps(x, unvoiced_value)
                        bad |= status.cpu().numpy()
                    dev.append((x, wins, voiced))
                out = b.compose_ffo(dev).cpu().numpy()
                for k in np.nonzero(bad)[0]:
                    print("warning: %s: a column of an msd stream holds no valid value, %s is not written" % (
                        jobs[group[k]][0], jobs[group[k]][ns]), file=sys.stderr)
                stage.put(b, out, [None if bad[k] else jobs[i][ns] for k, i in enumerate(group)])
    return stage.frames


# ---- the acoustic model's input rows from labels (data/scripts/makefeature.pl, Training.pl:1677-1723) ----------------
_INTEGER = re.compile(rb"^[+-]?[0-9]+$")
_LEADING_NUMBER = re.compile(rb"^\s*[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?")


def parse_question_config(text):
    """makefeature.pl:63-180 on the text of a question config (str or bytes).  Returns (names, features): features is what
    world.LabelFeatureSet takes, a list of (kind, pattern, min, max) with kind 0 binary, 1 float, 2 .. 7 the reserved
    names in the script's order, pattern the text between the braces (None for a reserved feature), min = max = 0 for a
    binary feature.  Raises ValueError with the script's message where the script dies."""
    raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    reserved = [n.encode() for n in W.RESERVED_LABEL_FEATURES]
    names, features = [], []
    for line in raw.split(b"\n"):
        line = line.strip(b" \t\n\r\x0b\x0c")
        if not line or line.startswith(b"#"):
            continue
        shown = line.decode("latin-1")
        arr = line.split()
        name, kind, patt = arr[0], None, b""
        if name in reserved:
            kind = 2 + reserved.index(name)
        elif len(arr) > 1:
            kind = 1 if arr[1].find(b"%d") > 0 else 0
        if kind is None:
            raise ValueError("ERROR: Cannot specify feature type : " + shown)
        if kind <= 1 and arr[1].startswith(b"{") and arr[1].rfind(b"}") == len(arr[1]) - 1:
            patt = arr[1][1:-1]
        lo = hi = b""
        for field in arr[1 if kind >= 2 else 2 if kind == 1 else 0:]:
            if field.startswith(b"MIN="):
                lo = field[4:]
            elif field.startswith(b"MAX="):
                hi = field[4:]
        if kind <= 1 and patt == b"":
            raise ValueError("ERROR: There is not feature patten : " + shown)
        if kind == 1:
            if patt.find(b"%d") < 0:
                raise ValueError("ERROR: There is not '%d' in feature pattern : " + shown)
            if patt.find(b"%d") != patt.rfind(b"%d"):
                raise ValueError("ERROR: There are multiple '%d' in feature pattern : " + shown)
            if b"," in patt:
                raise ValueError("ERROR: There are multiple patterns for float in feature pattern : " + shown)
        if kind >= 1:
            if lo == b"" or hi == b"":
                raise ValueError("ERROR: Min and max values are required : " + shown)
            if not _INTEGER.match(lo) or not _INTEGER.match(hi):
                raise ValueError("ERROR: Min and max values must be integer : " + shown)
        names.append(name.decode("latin-1"))
        features.append((kind, patt.decode("latin-1") if kind <= 1 else None, int(lo) if kind >= 1 else 0,
                         int(hi) if kind >= 1 else 0))
    return names, features


def read_question_config(path):
    """parse_question_config on a file."""
    with open(path, "rb") as f:
        return parse_question_config(f.read())


def _perl_number(field):
    m = _LEADING_NUMBER.match(field)                   # Perl's numeric value of a string: its leading number, else 0
    return float(m.group(0)) if m else 0.0


def parse_label(text, frame_shift):
    """makefeature.pl:194-289 on the text of a label file; frame_shift in the label's time unit (100 ns, as
    Training.pl:1685 passes it).  Returns (lines, state_level): lines a list of (start, end, name, state_index) with
    start = int(0.5 + field 0 / frame_shift), end likewise, the state index the integer >= 2 between the name's last `[`
    and its last character (else 0) and the name cut at that `[`; state_level whether the FIRST line had one.  A
    phoneme-level line in a state-level file raises; a state-level line in a phoneme-level file is accepted with its name
    cut, as the script's misspelt level check lets it through.  Raises ValueError with the script's message where the
    script dies."""
    raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    body = raw.split(b"\n")
    if body and body[-1] == b"":
        body.pop()                                     # the text after the last newline is a line only if there is some
    lines, level = [], None
    for line in body:
        line = line.strip(b" \t\n\r\x0b\x0c")
        shown = line.decode("latin-1")
        arr = line.split()
        if len(arr) < 2:
            raise ValueError("ERROR: There is not start/end time in label : " + shown)
        start, end = (0.5 + _perl_number(f) / frame_shift for f in arr[:2])
        if not (abs(start) < 1e15 and abs(end) < 1e15):
            raise ValueError("ERROR: Start/end must be integer in label : " + shown)
        start, end = int(start), int(end)
        name = arr[2] if len(arr) > 2 else b""
        left, right, state = name.rfind(b"["), name.rfind(b"]"), 0
        if 0 < left < right:
            inner = name[left + 1:-1]
            if _INTEGER.match(inner) and int(inner) >= 2:
                state = int(inner)
                name = name[:left]
        if end <= start or start < 0:
            raise ValueError("ERROR: There is error of start/end value in label : " + shown)
        if name == b"":
            raise ValueError("ERROR: There is not model name in label : " + shown)
        if level is None:
            level = state > 0
        elif level and state == 0:
            raise ValueError("ERROR: There is phoneme-level line in state-level label : " + shown)
        lines.append((start, end, name.decode("latin-1"), state))
    if level is None:
        raise ValueError("ERROR: Unknown label level")
    return lines, level


def read_label(path, frame_shift):
    """parse_label on a file."""
    with open(path, "rb") as f:
        return parse_label(f.read(), frame_shift)


def ffi_files(jobs, config, frame_shift, ctx=None, max_batch_frames=MAX_BATCH_FRAMES, io_threads=8, resume=False):
    """make_train_data_dnn / make_gen_data_dnn (scripts/Training.pl:1677-1723) for a file list: `makefeature.pl config
    frame_shift label | x2x +af > ffi`.

    jobs:   [(label_file, ffi_out)]; ffi_out: float32 [T][n_features], T the sum of the lines' end - start (no header)
    config: the question config's path, or what parse_question_config returned
    frame_shift: in 100 ns units, as Training.pl:1685 passes it
    Rank-sharded by frame count; with resume, utterances whose ffi file is complete are skipped.  Where the script warns,
    the utterances are counted per kind and the counts printed on stderr ("Out of range": a value was clamped to 0 or 1;
    "There is not state-level information in label").  Returns the frames written."""
    jobs = list(jobs)
    if any(len(j) != 2 for j in jobs):
        raise ValueError("ffi_files: a job is (label_file, ffi_out)")
    names, features = read_question_config(config) if isinstance(config, (str, os.PathLike)) else config
    nf = len(features)
    if nf < 1:
        raise ValueError("ffi_files: the question config holds no feature")
    labels = [read_label(j[0], frame_shift) for j in jobs]
    frames = [sum(e - s for s, e, _, _ in lines) for lines, _ in labels]
    mine = _my_jobs(frames, lambda i: not (resume and _size_is(jobs[i][1], 4 * nf * frames[i])))
    if not mine:
        return 0
    clamped, no_state = 0, 0
    with _Stage(ctx, io_threads) as stage, contextlib.closing(W.LabelFeatureSet(stage.ctx, features)) as fset:
        for group, batch in stage.batches(mine, frames, max_batch_frames):
            with batch as b:
                out, status = b.label_features(fset, [labels[i] for i in group])
                rows, status = out.cpu().numpy(), status.cpu().numpy()
                stage.put_native(b, [(rows, [jobs[i][1] for i in group])], io_threads)
                clamped += int((status & 1 != 0).sum())
                no_state += int((status & 2 != 0).sum())
    print("warnings: Out of range in %d utterances, no state-level information in %d" % (clamped, no_state), file=sys.stderr)
    return stage.frames


def stats_files(ffo_paths, streams, out_dir, names=("mgc", "lf0", "bap", "vib"), ctx=None,
                max_batch_frames=MAX_BATCH_FRAMES, io_threads=8):
    """The recipe's `stats` stage (data/Makefile.in:414-459) over a list of ffo files.

    ffo_paths: float32 files [T][row width] in the layout of `streams` (ffo_layout), what ffo_files writes
    Writes out_dir/ffo.var: one float32 row, the variance of every ffo column over all frames of all files (`cat ffo/* |
    vstat -d -o 2`, :440), the row gen_param_files takes as var_path; <name>.var per stream: its mean columns of that
    row (:441-443), names in the streams' order; gv.var: the variance across utterances of the per-utterance variances
    (:446-449), cut to the static columns of every stream in order (:454-456).
    Variances divide by n: the reading of `vstat -o 2` that the modulation-spectrum statistics took.  SPTK is not
    available to this project's tests, so the divisor is unconfirmed.  The reference guards its `stats` target so that
    it runs only without WORLD or STRAIGHT (:416) and its row leaves out `vib`; here the layout is taken from `streams`.
    The moments come per utterance from the device (count, mean, sum of squared deviations: never sum x^2) and are
    pooled on the host in path order (world.pool_moments).  Rank-sharded by frame count: each rank pools its shard --
    the moments, and a second triple over its per-utterance variances with count 1 each -- the triples are gathered
    and merged in rank order, and rank 0 writes; several ranks need an initialised process group.  Returns the frames
    counted."""
    import torch
    paths = [str(p) for p in ffo_paths]
    streams = _streams_arg(streams)
    layout, width = ffo_layout(streams)
    if len(names) < len(streams):
        raise ValueError("stats_files: %d streams but %d names" % (len(streams), len(names)))
    frames = [_rows_in((p,), width) for p in paths]
    mine = sorted(_my_jobs(frames, lambda i: frames[i] > 0))          # a batch holds no utterance without frames
    rank, world = _rank_world()
    at = {i: k for k, i in enumerate(mine)}
    cnt = np.zeros((len(mine), width), dtype=np.int64)
    mean, m2 = np.zeros((len(mine), width)), np.zeros((len(mine), width))
    if mine:
        with _Stage(ctx, io_threads) as stage:
            for group in stage.groups(mine, frames, max_batch_frames):
                rows = stage.load([paths[i] for i in group], width)
                with stage.batch(f0_lengths=[frames[i] for i in group]) as b:
                    c_, m_, s_ = (t.cpu().numpy() for t in b.column_moments(rows))
                sel = [at[i] for i in group]
                cnt[sel], mean[sel], m2[sel] = c_, m_, s_
    corpus = W.pool_moments(cnt, mean, m2)                            # over frames
    gv = W.pool_moments(np.ones_like(cnt), m2 / np.maximum(cnt, 1), np.zeros_like(m2))     # over utterances
    if world > 1:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("stats_files with WORLD_SIZE > 1 needs torch.distributed to be initialised: the ranks' "
                               "moments have to be merged")
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        packed = torch.from_numpy(np.stack([a.astype(np.float64) for a in corpus + gv])).to(dev)    # counts < 2^53
        parts = [torch.empty_like(packed) for _ in range(world)]
        dist.all_gather(parts, packed)
        parts = np.stack([p.cpu().numpy() for p in parts])            # [rank][6][width]
        corpus = W.pool_moments(parts[:, 0].astype(np.int64), parts[:, 1], parts[:, 2])
        gv = W.pool_moments(parts[:, 3].astype(np.int64), parts[:, 4], parts[:, 5])
    n = int(corpus[0].max()) if width else 0
    if rank == 0 and n > 0:
        os.makedirs(str(out_dir), exist_ok=True)
        var = (corpus[2] / corpus[0]).astype(np.float32)
        var.tofile(os.path.join(str(out_dir), "ffo.var"))
        gvar = (gv[2] / gv[0]).astype(np.float32)
        for name, (_, c0, cols) in zip(names, layout):
            var[c0:c0 + cols].tofile(os.path.join(str(out_dir), "%s.var" % name))
        np.concatenate([gvar[c0:c0 + dim] for (_, c0, _), (dim, _, _) in zip(layout, streams)]).tofile(
            os.path.join(str(out_dir), "gv.var"))
    return n


def gv_data_files(jobs, streams, sampling_rate, frame_shift, silences=(), unvoiced_value=-1.0e10, ctx=None,
                  max_batch_frames=MAX_BATCH_FRAMES, io_threads=8, resume=False):
    """`make_data_gv` (scripts/Training.pl:1402-1491) for a file list: the per-utterance variance vectors that GV
    training reads (gv/data/<base>.cmp).

    jobs:     [(stream_file_0, ..., stream_file_k, label_file or None, cmp_out)] -- the streams' FEATURE files, float32
              [T][dim_s]
    streams:  [(dim_s, windows, msd)]: the triple of ffo_files; the windows are not used
    sampling_rate, frame_shift: addhtkheader.pl's SAMPFREQ and FRAMESHIFT (samples); a frame is frame_shift /
              sampling_rate seconds
    silences: label names to drop ($nosilgv, :1422-1440); the rows kept are mspf_label_rows' (both ends inclusive)
    Per utterance the variance (dividing by n, see stats_files) of every column of every stream; in a stream with msd,
    values equal to unvoiced_value are dropped.  The script's `grep -v` drops single values and so shifts the columns of
    a two-column stream when only one of them carries the value; here every column is counted on its own.  The output
    is one HTK vector: htk_header(1, sampling_rate, frame_shift, 4 * sum dim, 9) and the float32 row (:1453).  An
    utterance with a column without values or a variance that is not finite is reported on stderr and not written
    (:1454-1458).  Rank-sharded by frame count; with resume, utterances whose file is complete are not computed again.
    Returns the list of written (or, with resume, complete) paths of this rank in job order: the script's scp."""
    jobs = [tuple(j) for j in jobs]
    streams = _streams_arg([(d, ws if ws else [[1.0]], m) for d, ws, m in streams])
    ns = len(streams)
    dims = [d for d, _, _ in streams]
    silences = tuple(silences)
    shift_s = float(frame_shift) / float(sampling_rate)
    frames = _stream_frames(jobs, dims, ns + 2, "%d stream files, a label and one output path" % ns)
    size_out = 12 + 4 * sum(dims)
    have = [resume and _size_is(j[ns + 1], size_out) for j in jobs]
    mine = _my_jobs(frames, lambda i: not have[i])
    written = {i for i in range(len(jobs)) if have[i] and _rank_world()[0] == 0}

    def skip(i, why):
        print("warning: %s: %s, %s is not written" % (jobs[i][0], why, jobs[i][ns + 1]), file=sys.stderr)

    for i in [i for i in mine if frames[i] == 0]:
        skip(i, "no frames")
    mine = [i for i in mine if frames[i] > 0]
    if mine:
        with _Stage(ctx, io_threads) as stage:
            head = W.htk_header(1, sampling_rate, frame_shift, 4 * sum(dims), 9)
            for group in stage.groups(mine, frames, max_batch_frames):
                keep = []
                for i in group:
                    if silences and jobs[i][ns]:
                        with open(jobs[i][ns]) as f:
                            keep.append(mspf_label_rows(f.readlines(), shift_s, frames[i], silences))
                    else:
                        keep.append(np.arange(frames[i], dtype=np.int64))
                left = [k for k in range(len(group)) if len(keep[k]) > 0]
                for k in range(len(group)):
                    if len(keep[k]) == 0:
                        skip(group[k], "no frames outside the silences")
                if not left:
                    continue
                off = np.concatenate([[0], np.cumsum([frames[i] for i in group])])
                index = _upload(np.concatenate([keep[k] + off[k] for k in left]))
                var, cnt = [], []
                with stage.batch(W.default_params(sampling_rate, 5.0), f0_lengths=[len(keep[k]) for k in left]) as b:
                    for s_, (dim, _, msd) in enumerate(streams):
                        x = stage.load([jobs[i][s_] for i in group], dim)[index].contiguous()
                        c_, _, s2 = b.column_moments(x, ignore_value=unvoiced_value if msd else None)
                        cnt.append(c_.cpu().numpy())
                        var.append(s2.cpu().numpy() / np.maximum(cnt[-1], 1))
                cnt, var = np.concatenate(cnt, axis=1), np.concatenate(var, axis=1).astype(np.float32)
                for r, k in enumerate(left):
                    i = group[k]
                    if (cnt[r] == 0).any():
                        skip(i, "a column without values")
                    elif not np.isfinite(var[r]).all():
                        skip(i, "a variance that is not finite")
                    else:
                        stage.submit(_put, jobs[i][ns + 1], var[r], head)
                        written.add(i)
    return [jobs[i][ns + 1] for i in sorted(written)]


# ---- mel-cepstral postfilter (scripts/Training.pl:2642-2687 postfiltering_mcp) ----------------------------------------
def postfilter_files(jobs, order, alpha, beta=1.4, length=4096, ctx=None, max_batch_frames=MAX_BATCH_FRAMES,
                     io_threads=8, resume=False):
    """`postfiltering_mcp` (scripts/Training.pl:2642-2687) for a file list, as gen_wave runs it on every generated
    `.mgc` (:2838-2840) before mgc2sp.

    jobs:  [(mgc_in, p_mgc_out)] -- float32 [T][order+1] in, float32 of the same shape out ($base.p_mgc)
    alpha, beta, length: $fw, $pf_mcp, $fl of the recipe's configuration
    The rows go to the device as float32 and are widened there; the result is rounded to float32 once, where the script
    rounds at every pipe.  Rank-sharded by frame count; with resume, utterances whose output has the input's size are
    skipped."""
    jobs = list(jobs)
    width = int(order) + 1
    frames = [_rows_in(j, width, 2, "one output path") for j in jobs]
    mine = _my_jobs(frames, lambda i: not (resume and _size_is(jobs[i][1], 4 * width * frames[i])))
    if not mine:
        return 0
    with _Stage(ctx, io_threads) as stage:
        for group, batch in stage.batches(mine, frames, max_batch_frames):
            with batch as b:
                rows = stage.load([jobs[i][0] for i in group], width)
                out, status = b.postfilter_mel_cepstrum(rows.double(), alpha, beta, length)
                host = out.float().cpu().numpy()
                st = status.cpu().numpy()
                fo = b.frame_offsets
                for k, i in enumerate(group):
                    bad = np.nonzero(st[fo[k]:fo[k + 1]])[0]
                    if len(bad):
                        print("warning: %s: %d frames flagged (first: frame %d, status %d), written as zeros" % (
                            jobs[i][0], len(bad), int(bad[0]), int(st[fo[k] + bad[0]])), file=sys.stderr)
                stage.put(b, host, [jobs[i][1] for i in group])
    return stage.frames


# ---- conversion between mel-generalized cepstra (SPTK's mgc2mgc: scripts/Training.pl:2861-2868, :2702-2705) ---------
def sptk_gamma(g=None, c=None):
    """SPTK's two ways to name a gamma: -g G as it is, -c N as -1 / N (N >= 1); neither: 0."""
    if g is not None and c is not None:
        raise ValueError("gamma is given by -g or by -c, not both")
    if c is not None:
        if c < 1:
            raise ValueError("-c %d: at least 1" % c)
        return -1.0 / c
    return 0.0 if g is None else float(g)


def mgc2mgc_check(order, alpha, gamma, out_order, out_alpha, out_gamma, multiplied=False, out_multiplied=False):
    """ValueError for what WorldMi355MelGeneralizedCepstrumConvert refuses, before a file is read."""
    if not (1 <= order <= 4095 and 1 <= out_order <= 4095 and min(order, out_order) <= 63):
        raise ValueError("orders %d -> %d: 1 .. 4095 each, one of them at most 63" % (order, out_order))
    if not (abs(alpha) < 1 and abs(out_alpha) < 1 and -1 <= gamma <= 1 and -1 <= out_gamma <= 1):
        raise ValueError("|alpha| < 1 and -1 <= gamma <= 1 on both sides")
    if (multiplied and gamma == 0) or (out_multiplied and out_gamma == 0):
        raise ValueError("-u needs gamma != 0 on the input side, -U on the output side")


def mgc2mgc_files(jobs, order, alpha, gamma, out_order, out_alpha, out_gamma, normalized=False, multiplied=False,
                  out_normalized=False, out_multiplied=False, ctx=None, max_batch_frames=MAX_BATCH_FRAMES, io_threads=8,
                  resume=False):
    """SPTK's `mgc2mgc -m order -a alpha -g gamma [-n] [-u] -M out_order -A out_alpha -G out_gamma [-N] [-U]` for a
    file list: the step gen_wave (scripts/Training.pl:2861-2868) and postfiltering_lsp (:2702-2705, :2739-2742) take
    with GAMMA != 0 (flag semantics unpinned against SPTK's command: include/world_mi355.h is the definition).

    jobs:  [(in, out)] -- float32 [T][order+1] in, float32 [T][out_order+1] out
    SPTK's file contract: the rows are widened to double on the device, converted there, and rounded to float32 once on
    the way out.  Rank-sharded by frame count; with resume, utterances whose output has its full size are skipped."""
    jobs = list(jobs)
    mgc2mgc_check(order, alpha, gamma, out_order, out_alpha, out_gamma, multiplied, out_multiplied)
    width, out_width = int(order) + 1, int(out_order) + 1
    frames = [_rows_in(j, width, 2, "one output path") for j in jobs]
    mine = _my_jobs(frames, lambda i: not (resume and _size_is(jobs[i][1], 4 * out_width * frames[i])))
    if not mine:
        return 0
    with _Stage(ctx, io_threads) as stage:
        # the limit counts rows of at most 64 coefficients: rows of up to 4096 take their share of it
        limit = max(1, max_batch_frames * 64 // max(64, width, out_width))
        for group, batch in stage.batches(mine, frames, limit):
            with batch as b:
                rows = stage.load([jobs[i][0] for i in group], width)
                out, status = b.convert_mel_generalized_cepstrum(rows.double(), alpha, gamma, out_order, out_alpha,
                                                                 out_gamma, normalized, multiplied, out_normalized,
                                                                 out_multiplied)
                host = out.float().cpu().numpy()
                st = status.cpu().numpy()
                fo = b.frame_offsets
                for k, i in enumerate(group):
                    bad = np.nonzero(st[fo[k]:fo[k + 1]])[0]
                    if len(bad):
                        print("warning: %s: %d frames flagged (first: frame %d, status %d), written as zeros" % (
                            jobs[i][0], len(bad), int(bad[0]), int(st[fo[k] + bad[0]])), file=sys.stderr)
                stage.put(b, host, [jobs[i][1] for i in group])
    return stage.frames


# ---- MGC-LSP rows to MGC rows and the LSP postfilter (scripts/Training.pl:2861-2868, :2690-2752) -----------------------
def lsp_check(order, alpha, gamma, out_order=None, out_alpha=None, out_gamma=None, beta=None, length=None):
    """ValueError for what WorldMi355LspToMelGeneralizedCepstrum (beta None) or WorldMi355LspPostfilter refuses, before a
    file is read."""
    if not 1 <= order <= 63:
        raise ValueError("order %d: 1 .. 63" % order)
    if not (abs(alpha) < 1 and -1 <= gamma < 0):
        raise ValueError("|alpha| < 1 and -1 <= gamma < 0: MGC-LSP rows exist at gamma != 0 only")
    if beta is None:
        mgc2mgc_check(order, alpha, gamma, order if out_order is None else out_order,
                      alpha if out_alpha is None else out_alpha, gamma if out_gamma is None else out_gamma, True)
        return
    if not np.isfinite(beta):
        raise ValueError("beta must be finite")
    if not (64 <= length <= 4096 and length & (length - 1) == 0):
        raise ValueError("length %d: a power of two, 64 .. 4096" % length)


def _lsp_stage(jobs, order, out_width, call, ctx, max_batch_frames, io_threads, resume):
    """The file loop of lsp2mgc_files and postfilter_lsp_files: float32 [T][order+1] in, float32 [T][out_width] out of
    call(batch, float64 rows) -> (rows, status)."""
    jobs = list(jobs)
    width = int(order) + 1
    frames = [_rows_in(j, width, 2, "one output path") for j in jobs]
    mine = _my_jobs(frames, lambda i: not (resume and _size_is(jobs[i][1], 4 * out_width * frames[i])))
    if not mine:
        return 0
    with _Stage(ctx, io_threads) as stage:
        for group, batch in stage.batches(mine, frames, max_batch_frames):
            with batch as b:
                rows = stage.load([jobs[i][0] for i in group], width)
                out, status = call(b, rows.double())
                host = out.float().cpu().numpy()
                st = status.cpu().numpy()
                fo = b.frame_offsets
                for k, i in enumerate(group):
                    bad = np.nonzero(st[fo[k]:fo[k + 1]] & 12)[0]
                    if len(bad):
                        print("warning: %s: %d frames flagged (first: frame %d, status %d), written as zeros" % (
                            jobs[i][0], len(bad), int(bad[0]), int(st[fo[k] + bad[0]])), file=sys.stderr)
                stage.put(b, host, [jobs[i][1] for i in group])
    return stage.frames


def lsp2mgc_files(jobs, order, alpha, gamma, log_gain=False, out_order=None, out_alpha=None, out_gamma=None, ctx=None,
                  max_batch_frames=MAX_BATCH_FRAMES, io_threads=8, resume=False):
    """gen_wave's `lspcheck -c -r 0.1 -g -G 1e-10 | lsp2lpc | mgc2mgc -n -u` (scripts/Training.pl:2861-2868) for a file
    list: MGC-LSP rows [gain, lsp_1 .. lsp_m] to plain MGC rows (lsp.lsp_to_mel_generalized_cepstrum; include/world_mi355.h
    is the definition, parity with SPTK's lspcheck and lsp2lpc is unpinned).

    jobs:  [(in, c_mgc_out)] -- float32 [T][order+1] in, float32 [T][out_order+1] out
    out_order, out_alpha, out_gamma: None for the input's own, which is gen_wave's call.
    The rows are widened to double on the device and rounded to float32 once on the way out.  Rank-sharded by frame
    count; with resume, utterances whose output has its full size are skipped."""
    from . import lsp as L
    lsp_check(order, alpha, gamma, out_order, out_alpha, out_gamma)
    out_width = int(order if out_order is None else out_order) + 1
    return _lsp_stage(jobs, order, out_width,
                      lambda b, rows: L.lsp_to_mel_generalized_cepstrum(b, rows, alpha, gamma, out_order, out_alpha,
                                                                        out_gamma, log_gain),
                      ctx, max_batch_frames, io_threads, resume)


def postfilter_lsp_files(jobs, order, alpha, gamma, beta=0.7, length=4096, log_gain=False, compensate=False, ctx=None,
                         max_batch_frames=MAX_BATCH_FRAMES, io_threads=8, resume=False):
    """`postfiltering_lsp` (scripts/Training.pl:2690-2752) for a file list, the step gen_wave takes on MGC-LSP rows
    where it takes postfiltering_mcp on mel-cepstra (:2846-2860).

    jobs:  [(in, p_mgc_out)] -- float32 [T][order+1] in, float32 of the same shape out
    beta, length: $pf_lsp, $fl.  compensate: put the energy difference into the gain, which the script as written does
    not (lsp.postfilter_lsp).  Rank-sharded by frame count; with resume, utterances whose output has the input's size
    are skipped."""
    from . import lsp as L
    lsp_check(order, alpha, gamma, beta=beta, length=length)
    return _lsp_stage(jobs, order, int(order) + 1,
                      lambda b, rows: L.postfilter_lsp(b, rows, alpha, gamma, beta, length, compensate, log_gain),
                      ctx, max_batch_frames, io_threads, resume)


# ---- mel-cepstra from waveforms (data/Makefile.in:134-137: x2x +sf | frame | window | mgcep at gamma 0) ---------------
def read_samples(path):
    """The int16 values of a headerless little-endian `.raw` file (what `x2x +sf` reads) or of a 16-bit wav, as float64
    and as they are: SPTK's pipe carries them undivided."""
    if str(path).lower().endswith(".raw"):
        return np.fromfile(str(path), dtype="<i2").astype(np.float64)
    x, _ = read_wav(path)
    return x * 32768.0                                      # read_wav divided the 16-bit values by 2^15: exact both ways


def _sample_count(path):
    if str(path).lower().endswith(".raw"):
        size = os.path.getsize(str(path))
        if size % 2:
            raise ValueError("%s: %d bytes are no int16 samples" % (path, size))
        return size // 2
    with wave.open(str(path), "rb") as w:
        if w.getsampwidth() != 2:
            raise ValueError("%s: mgcep takes 16-bit samples, the file has %d-bit ones" % (path, 8 * w.getsampwidth()))
        return w.getnframes()


def mgcep_check(frame_length, frame_shift, fft_length, window, normalize, alpha, order, eps, max_batch_frames=1):
    """What mgcep_files refuses, as a ValueError, before anything is opened."""
    if fft_length not in (512, 1024, 2048, 4096):
        raise ValueError("fft_length %r: 512, 1024, 2048 or 4096" % (fft_length,))
    if not 2 <= frame_length <= fft_length:
        raise ValueError("frame_length %r: from 2 to fft_length = %d" % (frame_length, fft_length))
    if not 1 <= frame_shift <= frame_length:
        raise ValueError("frame_shift %r: from 1 to frame_length = %d" % (frame_shift, frame_length))
    if window not in (0, 1, 2, 5):
        raise ValueError("window %r: 0 Blackman, 1 Hamming, 2 Hanning or 5 rectangular" % (window,))
    if normalize not in (0, 1, 2):
        raise ValueError("normalize %r: 0 none, 1 power or 2 magnitude" % (normalize,))
    if not 1 <= order <= 63:
        raise ValueError("order %r: from 1 to 63" % (order,))
    if not abs(alpha) < 1.0:
        raise ValueError("alpha %r: |alpha| < 1" % (alpha,))
    if not eps >= 0.0:
        raise ValueError("eps %r: a value >= 0 added to the periodogram" % (eps,))
    if max_batch_frames < 1:
        raise ValueError("max_batch_frames %r: at least 1" % (max_batch_frames,))


def mgcep_files(jobs, frame_length=1200, frame_shift=240, fft_length=2048, window=1, normalize=1, alpha=0.55, order=49,
                eps=1.0e-8, itr1=2, itr2=30, dd=1.0e-3, pipe_float32=True, ctx=None, max_batch_frames=MAX_BATCH_FRAMES,
                io_threads=8, resume=False):
    """The recipe's spectral analysis without WORLD (data/Makefile.in:134-137, the default USEWORLD=0, GAMMA=0) for a file
    list: `x2x +sf raw | frame -l frame_length -p frame_shift | window -l frame_length -L fft_length -w window -n
    normalize | mgcep -a alpha -m order -l fft_length -e eps > mgc`, in one kernel per batch (mel_cepstrum_of_waveform).

    jobs:  [(raw_or_wav, mgc_out)] -- `.raw`: headerless little-endian int16; anything else: a 16-bit wav.  The samples
           are the int16 values as they are.  Out: float32 [J][order+1], J = sptk_frames(samples).
    pipe_float32: the windowed samples are rounded to float32 once, as the pipe between `window` and `mgcep` does.
    An utterance with a frame of status 1 or 2 (theq's singular pivot, a periodogram value that is not positive and
    finite) is reported on stderr and its file is not written -- the recipe's $(NAN) check (:152-155); status -1 is mcep's
    ordinary return.  Rank-sharded by frame count; batches close at max_batch_frames; with resume, utterances whose
    output has the complete size are skipped.  Returns (frames analysed by this rank, the flagged inputs)."""
    mgcep_check(frame_length, frame_shift, fft_length, window, normalize, alpha, order, eps, max_batch_frames)
    import torch  # noqa: F401 -- ahead of the first call into the library (analysis_files says why)
    jobs = list(jobs)
    width = int(order) + 1
    with ThreadPoolExecutor(io_threads) as pool:
        samples = list(pool.map(lambda j: _sample_count(j[0]), jobs))
    empty = [jobs[i][0] for i, n in enumerate(samples) if n == 0]
    if empty:
        raise ValueError("%s holds no samples" % empty[0])
    frames = [W.sptk_frames(n, frame_length, frame_shift) for n in samples]
    mine = _my_jobs(frames, lambda i: not (resume and _size_is(jobs[i][1], 4 * width * frames[i])))
    flagged = []
    if not mine:
        return 0, flagged
    table = W.sptk_window(window, normalize, frame_length)
    params = W.default_params(48000, 5.0, fft_size=fft_length)     # of the batch only fft_size is read
    with _Stage(ctx, io_threads) as stage:
        for group in stage.groups(mine, frames, max_batch_frames):
            xs = list(stage.pool.map(lambda i: read_samples(jobs[i][0]), group))
            with stage.batch(params, x_lengths=[len(x) for x in xs], f0_lengths=[frames[i] for i in group]) as b:
                x = _upload(np.concatenate(xs), pinned=True)
                del xs
                mc, status = b.mel_cepstrum_of_waveform(x, table, frame_length, frame_shift, order, alpha, pipe_float32,
                                                        etype=1, e=eps, itr1=itr1, itr2=itr2, dd=dd)
                host = mc.float().cpu().numpy()
                st = status.cpu().numpy()
                fo = b.frame_offsets
                paths = []
                for k, i in enumerate(group):
                    bad = np.nonzero(st[fo[k]:fo[k + 1]] > 0)[0]
                    if len(bad):
                        print("warning: %s: %d frames flagged (first: frame %d, status %d), not written" % (
                            jobs[i][0], len(bad), int(bad[0]), int(st[fo[k] + bad[0]])), file=sys.stderr)
                        flagged.append(jobs[i][0])
                    paths.append(None if len(bad) else jobs[i][1])
                stage.put(b, host, paths)
    return stage.frames, flagged


# ---- waveforms from mel-cepstra (scripts/Training.pl:2873-2899: excite | dfs | vopr -a | mglsadf | x2x +fs -o) ----------
def read_taps(text_or_path):
    """The taps `dfs -b` takes, from the text data/scripts/makefilter.pl prints (numbers separated by blanks) or from a
    file that holds it."""
    text = str(text_or_path)
    if os.path.exists(text):
        with open(text) as f:
            text = f.read()
    try:
        taps = np.array([float(t) for t in text.split()], dtype=np.float64)
    except ValueError:
        raise ValueError("%r: neither a file nor numbers separated by blanks" % (text_or_path,))
    if not 1 <= len(taps) <= 256 or not np.isfinite(taps).all():
        raise ValueError("%r: 1 to 256 finite taps, got %d" % (text_or_path, len(taps)))
    return taps


def mlsa_pitch(lf0, fs):
    """`sopr -magic -1.0E+10 -EXP -INV -m fs -MAGIC 0.0` on float32 lf0: the period in samples, in double and rounded to
    float32 once; 0 for the magic value."""
    lf0 = np.asarray(lf0, dtype=np.float32)
    voiced = lf0 != np.float32(-1.0e10)
    pitch = np.zeros(lf0.shape, dtype=np.float64)
    pitch[voiced] = float(fs) * (1.0 / np.exp(lf0[voiced].astype(np.float64)))
    return pitch.astype(np.float32)


def pcm16_of_pipe(y):
    """`x2x +fs -o`: clipped to [-32768, 32767] and truncated toward zero (this reading of -o is unpinned: SPTK is not in
    the reference tree)."""
    return np.trunc(np.clip(np.asarray(y, dtype=np.float64), -32768.0, 32767.0)).astype("<i2")


def _put_raw_and_wav(raw_path, wav_path, pcm, fs):
    pcm.tofile(raw_path)
    n = len(pcm)
    head = b"RIFF" + struct.pack("<I", 36 + n * 2) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, fs, fs * 2, 2, 16)
    _put(wav_path, pcm, head + b"data" + struct.pack("<I", n * 2))


def mlsa_synth_check(fs, frame_shift, order, alpha, pade_order, max_batch_frames=2):
    """What mlsa_synth_files refuses, as a ValueError, before anything is opened."""
    if fs < 1:
        raise ValueError("fs %r: a sampling rate in Hz" % (fs,))
    if frame_shift < 1:
        raise ValueError("frame_shift %r: at least 1 sample" % (frame_shift,))
    if not 1 <= order <= 62:
        raise ValueError("order %r: from 1 to 62" % (order,))
    if not abs(alpha) < 1.0:
        raise ValueError("alpha %r: |alpha| < 1" % (alpha,))
    if not 1 <= pade_order <= 7:
        raise ValueError("pade_order %r: from 1 to 7" % (pade_order,))
    if max_batch_frames < 2:
        raise ValueError("max_batch_frames %r: at least 2" % (max_batch_frames,))


def mlsa_synth_files(jobs, lowpass, highpass, fs=48000, frame_shift=240, order=49, alpha=0.55, pade_order=5,
                     pipe_float32=True, pade=None, ctx=None, max_batch_frames=MAX_BATCH_FRAMES, io_threads=8,
                     resume=False):
    """gen_wave's first branch (scripts/Training.pl:2873-2899, the default USEWORLD=0, GAMMA=0) for a file list:
    `sopr ... lf0 > pit`, `excite -n -p frame_shift | dfs -b`, `vopr -a`, `mglsadf -P pade_order -m order -p frame_shift
    -a alpha -c 0 mgc | x2x +fs -o > raw`, in one call per batch (mlsa_synthesis).

    jobs:  [(lf0, mgc, raw_out, wav_out)] -- float32 [T] with -1e10 for unvoiced and float32 [T][order+1] in; int16 and a
           16-bit wav of (T - 1) * frame_shift samples out.
    lowpass, highpass: the taps, as read_taps gives them (makefilter.pl's output for the sampling rate).
    pipe_float32: a value is rounded to float32 at each pipe of the shell line, as SPTK's float pipes do.
    The int16 conversion is pcm16_of_pipe's.  An utterance of status 1 (a non-finite coefficient, a non-finite or negative
    pitch) or 2 (a non-finite sample) is reported on stderr and its files are not written.  Rank-sharded by frame count;
    with resume, utterances whose two outputs have the complete sizes are skipped.  Returns (frames synthesised by this
    rank, the flagged lf0 inputs)."""
    mlsa_synth_check(fs, frame_shift, order, alpha, pade_order, max_batch_frames)
    import torch  # noqa: F401 -- ahead of the first call into the library (analysis_files says why)
    lowpass, highpass = np.asarray(lowpass, dtype=np.float64), np.asarray(highpass, dtype=np.float64)
    jobs = list(jobs)
    width = int(order) + 1
    frames = [_rows_in(j, 1, 4, "lf0, mgc and the two output paths") for j in jobs]
    short = [jobs[i][0] for i, n in enumerate(frames) if n < 2]
    if short:
        raise ValueError("%s holds fewer than two frames" % short[0])
    samples = [W.mlsa_samples(n, frame_shift) for n in frames]
    mine = _my_jobs(frames, lambda i: not (resume and _size_is(jobs[i][2], 2 * samples[i])
                                           and _size_is(jobs[i][3], 44 + 2 * samples[i])))
    flagged = []
    if not mine:
        return 0, flagged
    with _Stage(ctx, io_threads) as stage:
        for group in stage.groups(mine, frames, max_batch_frames):
            with stage.batch(f0_lengths=[frames[i] for i in group], y_lengths=[samples[i] for i in group]) as b:
                want = [(frames[i], jobs[i][0]) for i in group]
                lf0 = list(stage.pool.map(lambda i: _f32(jobs[i][0]), group))
                pitch = _upload(np.concatenate([mlsa_pitch(a, fs) for a in lf0]))
                mc = stage.load([jobs[i][1] for i in group], width, want)
                y, status = b.mlsa_synthesis(pitch, mc, lowpass, highpass, order, alpha, pade_order, frame_shift,
                                             pipe_float32, pade)
                host = y.cpu().numpy()
                st = status.cpu().numpy()
                yo = b.out_offsets
                for k, i in enumerate(group):
                    if st[k]:
                        print("warning: %s: status %d, not written" % (jobs[i][0], int(st[k])), file=sys.stderr)
                        flagged.append(jobs[i][0])
                        continue
                    stage.submit(_put_raw_and_wav, jobs[i][2], jobs[i][3], pcm16_of_pipe(host[yo[k]:yo[k + 1]]), int(fs))
    return stage.frames, flagged


# ---- modulation-spectrum postfilter (scripts/Training.pl:2950-3038 postfiltering_mspf, :3133-3221 make_mspf) ----------
def mspf_label_rows(lines, frame_shift_s, n_rows, silences=()):
    """Rows that make_mspf's silence removal keeps: label lines "start end name" in 100 ns units; a segment's frames are
    int(start 1e-7 / shift) .. int(end 1e-7 / shift), both ends inclusive (`bcut -s -e`), clipped to the file, so
    adjacent segments repeat their boundary frame; segments named in `silences` are dropped, the rest butted together."""
    keep = []
    for line in lines:
        f = line.split()
        if len(f) < 3 or f[2] in silences:
            continue
        a = max(int(int(f[0]) * 1e-7 / frame_shift_s), 0)
        b = min(int(int(f[1]) * 1e-7 / frame_shift_s), n_rows - 1)
        keep.extend(range(a, b + 1))
    return np.asarray(keep, dtype=np.int64)


def _mspf_stat_paths(directory, name, d):
    base = os.path.join(str(directory), "%s_dim%d" % (name, d))
    return base + ".mean", base + ".stdd"


def mspf_stats_files(jobs, dim, out_dir, name="mgc", silences=(), frame_shift_s=0.005, frame_length=25, fft_length=64,
                     ctx=None, max_batch_frames=MAX_BATCH_FRAMES, io_threads=8):
    """`make_mspf` (scripts/Training.pl:3133-3221) for one side (natural or generated) of a file list.

    jobs:     [(feature_file, label_file or None)] -- float32 [T][dim] rows
    silences: label names to drop; with none (or no label file) the whole file is used.  With silence removal the mean
              is the whole file's and the kept segments are butted together (mspf_label_rows).
    Rank-sharded by frame count; the ranks' sums are added (all-reduce when a process group is up) and rank 0 writes
    out_dir/<name>_dim<d>.mean and .stdd, d = 0 .. dim-1, fft_length/2+1 float32 each.  Returns the frames counted."""
    import torch
    jobs = [tuple(j) for j in jobs]
    width, K = int(dim), int(fft_length) // 2 + 1
    silences = tuple(silences)
    frames = [_rows_in(j, width, 2, "one label path") for j in jobs]
    mine = _my_jobs(frames, lambda i: frames[i] > 0)                 # a batch holds no utterance without frames
    rank, world = _rank_world()
    s1 = torch.zeros(width, K, dtype=torch.float64)
    s2 = torch.zeros(width, K, dtype=torch.float64)
    count = 0
    if mine:
        with _Stage(ctx, io_threads) as stage:
            for group in stage.groups(mine, frames, max_batch_frames):
                rows = stage.load([jobs[i][0] for i in group], width).double()
                lengths, mean = [frames[i] for i in group], None
                if silences and any(jobs[i][1] for i in group):
                    with stage.batch(f0_lengths=lengths) as b:
                        mean = b.utterance_means(rows)
                    fo, keep, kept = b.frame_offsets, [], []
                    for k, i in enumerate(group):
                        if jobs[i][1]:
                            with open(jobs[i][1]) as f:
                                idx = mspf_label_rows(f.readlines(), frame_shift_s, frames[i], silences)
                        else:
                            idx = np.arange(frames[i], dtype=np.int64)
                        keep.append(idx + int(fo[k]))
                        kept.append(len(idx))
                    some_left = [k for k, n_ in enumerate(kept) if n_ > 0]      # all silence: nothing to count
                    if not some_left:
                        continue
                    rows = rows[_upload(np.concatenate(keep))].contiguous()
                    mean = mean[_upload(np.asarray(some_left, dtype=np.int64))].contiguous()
                    lengths = [kept[k] for k in some_left]
                with stage.batch(f0_lengths=lengths) as b:
                    a1, a2, n = b.modulation_spectrum_stats(rows, frame_length, fft_length, mean)
                    s1 += a1.cpu()
                    s2 += a2.cpu()
                    count += n
    if world > 1:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("mspf_stats_files with WORLD_SIZE > 1 needs torch.distributed to be initialised: the "
                               "ranks' sums have to be added")
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        packed = torch.cat([s1.flatten(), s2.flatten()]).to(dev)
        cnt = torch.tensor([count], dtype=torch.int64, device=dev)
        dist.all_reduce(packed)
        dist.all_reduce(cnt)
        packed = packed.cpu()
        s1, s2, count = packed[:width * K].view(width, K), packed[width * K:].view(width, K), int(cnt.item())
    if rank == 0 and count > 0:
        mean, std = W.mspf_finalize(s1.numpy(), s2.numpy(), count)
        os.makedirs(str(out_dir), exist_ok=True)
        for d in range(width):
            pm, ps = _mspf_stat_paths(out_dir, name, d)
            mean[d].astype(np.float32).tofile(pm)
            std[d].astype(np.float32).tofile(ps)
    return count


def mspf_files(jobs, dim, gen_stats_dir, nat_stats_dir, name="mgc", emphasis=1.0, frame_length=25, fft_length=64,
               ctx=None, max_batch_frames=MAX_BATCH_FRAMES, io_threads=8, resume=False):
    """`postfiltering_mspf` (scripts/Training.pl:2950-3038) for a file list, as gen_wave runs it with USEMSPF in the
    place of postfiltering_mcp.

    jobs:  [(mgc_in, p_mgc_out)] -- float32 [T][dim] in, float32 of the same shape out
    gen_stats_dir, nat_stats_dir: where mspf_stats_files wrote <name>_dim<d>.mean / .stdd for generated and natural
    parameters.  The rows are widened on the device and the result is rounded to float32 once.  Rank-sharded by frame
    count; with resume, utterances whose output has the input's size are skipped.  A flagged utterance is reported."""
    jobs = list(jobs)
    width, K = int(dim), int(fft_length) // 2 + 1
    frames = [_rows_in(j, width, 2, "one output path") for j in jobs]

    def table(directory, which):
        rows = [np.fromfile(_mspf_stat_paths(directory, name, d)[which], dtype=np.float32) for d in range(width)]
        if any(len(r) != K for r in rows):
            raise ValueError("%s: the %s statistics do not hold %d bins per dimension" % (directory, name, K))
        return np.stack(rows).astype(np.float64)

    todo = [not (resume and _size_is(j[1], 4 * width * frames[i])) for i, j in enumerate(jobs)]
    for i in [i for i in range(len(jobs)) if todo[i] and frames[i] == 0]:    # nothing to filter: the output is empty as well
        if _rank_world()[0] == 0:
            open(jobs[i][1], "wb").close()
    mine = _my_jobs(frames, lambda i: todo[i] and frames[i] > 0)
    if not mine:
        return 0
    tabs = (table(gen_stats_dir, 0), table(gen_stats_dir, 1), table(nat_stats_dir, 0), table(nat_stats_dir, 1))
    with _Stage(ctx, io_threads) as stage:
        for group, batch in stage.batches(mine, frames, max_batch_frames):
            with batch as b:
                rows = stage.load([jobs[i][0] for i in group], width)
                out, status = b.postfilter_modulation_spectrum(rows.double(), *tabs, emphasis, frame_length, fft_length)
                host = out.float().cpu().numpy()
                st = status.cpu().numpy()
                for k in np.nonzero(st)[0]:
                    print("warning: %s: flagged (status %d), the affected columns written as zeros" % (
                        jobs[group[k]][0], int(st[k])), file=sys.stderr)
                stage.put(b, host, [jobs[i][1] for i in group])
    return stage.frames


# ---- vibrato (data/scripts/Extract.py, data/Makefile.in:215) --------------------------------------------------------
_SCALE = ("C", "Db", "D", "Eb", "E", "F", "Gb", "G", "Ab", "A", "Bb", "B")


def note_pitch(note):
    """Hz of a note name such as "A4" or "Db5" (equal temperament around A4 = 440; Extract.py:109-114); 0 for "xx"."""
    if note == "xx":
        return 0.0
    return 440.0 * 2.0 ** (int(note[-1:]) - 4) * 2.0 ** ((_SCALE.index(note[:-1]) - 9) / 12.0)


def read_label_segments(mono_path, full_path, frame_period, n_frames):
    """[(start_frame, end_frame, note_pitch_hz)] of an utterance from its mono and full-context label files, as
    Extract.py reads them (:63-84, :176-187): three fields per line, times in units of 100 ns divided by 10e3 (ms),
    frames = floor(time / frame_period) clamped to [0, n_frames], the note from the `/E:<note>]` field of the
    full-context label."""
    with open(mono_path) as f:
        mono = f.read().split("\n")
    with open(full_path) as f:
        full = f.read().split("\n")
    if len(mono) != len(full):
        raise ValueError("mono label not equal with full label")
    out = []
    for m, fl in zip(mono, full):
        if m == "" or fl == "":
            continue
        md, fd = m.split(" "), fl.split(" ")
        if len(md) != 3 or len(fd) != 3:
            raise ValueError("label line without three fields")
        t0, t1 = float(md[0]) / 10e3, float(md[1]) / 10e3
        note = re.findall(r"/E:\w+\]", fd[2])[0].replace("/E:", "").replace("]", "")
        out.append((max(math.floor(t0 / frame_period), 0), min(math.floor(t1 / frame_period), n_frames), note_pitch(note)))
    return out


def vibrato_files(jobs, frame_period, fs=48000, ctx=None, max_batch_frames=MAX_BATCH_FRAMES, io_threads=8):
    """jobs: [(lf0_file, mono_label, full_label, vib_out)].  What `Extract.py <base> <frame_period>` does for every
    job: the lf0 file (float32 log f0, one column) is REWRITTEN with two columns (log f0, log(f0 - note + 500)), the
    vib file gets (log depth, log period) per frame.  fs only labels the batch (nothing here depends on it)."""
    jobs = list(jobs)
    frames = [os.path.getsize(j[0]) // 4 for j in jobs]
    mine = _my_share(frames)
    with _Stage(ctx, io_threads) as stage:
        for group, batch in stage.batches(mine, frames, max_batch_frames, W.default_params(fs, frame_period)):
            with batch as b:
                segs = [read_label_segments(jobs[i][1], jobs[i][2], frame_period, frames[i]) for i in group]
                vib, lf2, too_long = b.vibrato(stage.load([jobs[i][0] for i in group]), segs)
                if too_long:
                    print("warning: %d voiced run(s) longer than 3072 frames left without vibrato" % too_long, file=sys.stderr)
                vh, lh = vib.cpu().numpy(), lf2.cpu().numpy()
                stage.put(b, lh, [jobs[i][0] for i in group])
                stage.put(b, vh, [jobs[i][3] for i in group])
    return stage.frames


# ---- objective evaluation: generated against natural feature files (no counterpart in the recipe's scripts) -----------
EVAL_WORKSPACE_BYTES = 4 << 30                # a batch's alignment workspace stays below this where it holds several pairs


def parse_eval_stream(text):
    """`NAME:DIM` of evaluate's command line -> (name, dim), e.g. mgc:50."""
    name, _, dim = text.partition(":")
    if not name or not dim.isdigit() or int(dim) < 1:
        raise ValueError("a stream is NAME:DIM with DIM >= 1: " + text)
    return name, int(dim)


def evaluate_groups(streams, with_c0=False):
    """What evaluate scores of each stream, [(first column, count, kind)]: mgc is cepstral (kind 0) over the columns
    1 .. DIM-1, with_c0 adds column 0; lf0 is log f0 (kind 1, one column); any other stream is kind 0 over all columns."""
    groups = []
    for name, dim in streams:
        if name == "lf0":
            if dim != 1:
                raise ValueError("lf0 is one column, not %d" % dim)
            groups.append((0, 1, 1))
        elif name == "mgc" and not with_c0:
            if dim < 2:
                raise ValueError("mgc without c0 needs more than one column")
            groups.append((1, dim - 1, 0))
        else:
            groups.append((0, dim, 0))
    if any(c > 64 for _, c, _ in groups):
        raise ValueError("a stream is scored over at most 64 columns")
    return groups


def evaluate_files(jobs, streams, align="dtw", with_c0=False, silences=(), frame_shift_s=0.005, voiced_above=-1.0e9,
                   ctx=None, max_batch_frames=MAX_BATCH_FRAMES, max_workspace_bytes=EVAL_WORKSPACE_BYTES, io_threads=8):
    """Objective measures of generated against natural feature files (WorldBatch.dtw_align, feature_distortion).

    jobs:     [(generated_0, natural_0, generated_1, natural_1, ..., label file or None)]: per stream, in the streams'
              order, float32 rows of the stream's DIM; the natural utterance's label file last
    streams:  [(name, dim)]; what is scored of each: evaluate_groups
    align:    "dtw": the path is found on the mgc stream's scored columns and every stream is scored along it;
              "truncate": frame k against frame k up to the shorter side
    silences: label names whose frames of the NATURAL side are left out (gv_label_mask's rows, frame_shift_s seconds)
    Rank-sharded by cells (frames for truncate); a batch is closed by frames and, for dtw, by W.dtw_workspace_bytes.
    Returns (pooled, rows, info): pooled = W.pool_distortion's dict per stream, rows float64 [n_jobs][n_streams][4] in the
    jobs' order (zeros for a flagged utterance), info int64 [n_jobs][4] = T_a, T_b, pairs on the path, status.  With
    several ranks the rows are added up over the ranks, so every rank returns the same."""
    import torch
    if align not in ("dtw", "truncate"):
        raise ValueError("align is dtw or truncate, not %r" % (align,))
    streams = [(str(n_), int(d)) for n_, d in streams]
    groups = evaluate_groups(streams, with_c0)
    kinds = [k for _, _, k in groups]
    ns = len(streams)
    names = [n_ for n_, _ in streams]
    if align == "dtw" and "mgc" not in names:
        raise ValueError("--align dtw finds the path on the mgc stream: there is none")
    jobs = [tuple(j) for j in jobs]
    silences = tuple(silences)
    ta, tb = [], []
    for j in jobs:
        if len(j) != 2 * ns + 1:
            raise ValueError("%s: a job is %d paths (generated and natural per stream, the label file), not %d"
                             % (j[0], 2 * ns + 1, len(j)))
        sides = []
        for side in (0, 1):
            n = {_rows_in((j[2 * s + side],), d) for s, (_, d) in enumerate(streams)}
            if len(n) != 1:
                raise ValueError("%s: the streams' files disagree on the frames" % j[side])
            sides.append(n.pop())
        if not 1 <= sides[0] <= 32767 or sides[1] > 32767:
            raise ValueError("%s: %d generated and %d natural frames; 1 .. 32767 and 0 .. 32767 can be aligned"
                             % (j[0], sides[0], sides[1]))
        ta.append(sides[0])
        tb.append(sides[1])
    cost = [a_ * max(b_, 1) for a_, b_ in zip(ta, tb)] if align == "dtw" else ta
    mine = [k for k in _my_share(cost)]
    rank, world = _rank_world()
    rows = np.zeros((len(jobs), ns, 4), dtype=np.float64)
    info = np.zeros((len(jobs), 4), dtype=np.int64)
    fits = None
    if align == "dtw":
        fits = lambda g: W.dtw_workspace_bytes([ta[i] for i in g], [tb[i] for i in g]) <= max_workspace_bytes
    if mine:
        with _Stage(ctx, io_threads) as stage:
            order = sorted(mine, key=lambda i: -cost[i])
            for group in _batches(order, ta, max_batch_frames, fits):
                b_len = [tb[i] for i in group]
                with stage.batch(f0_lengths=[ta[i] for i in group]) as b:
                    gen = [stage.load([jobs[i][2 * s] for i in group], d) for s, (_, d) in enumerate(streams)]
                    nat = [stage.load([jobs[i][2 * s + 1] for i in group], d) if sum(b_len) else
                           torch.zeros(0, d, dtype=torch.float32, device="cuda") for s, (_, d) in enumerate(streams)]
                    mask = None
                    if silences and any(jobs[i][-1] for i in group):
                        parts = []
                        for i in group:
                            if jobs[i][-1]:
                                with open(jobs[i][-1]) as f:
                                    parts.append(gv_label_mask(f.readlines(), frame_shift_s, tb[i], silences))
                            else:
                                parts.append(np.ones(tb[i], dtype=np.uint8))
                        mask = _upload(np.concatenate(parts))
                    path = path_len = None
                    status = np.array([0 if n_ else 2 for n_ in b_len])
                    pairs = np.minimum([ta[i] for i in group], b_len)
                    if align == "dtw" and sum(b_len):
                        m = names.index("mgc")
                        path, path_len, _, st = b.dtw_align(gen[m], nat[m], b_len, groups[m][0], groups[m][1])
                        status, pairs = st.cpu().numpy(), path_len.cpu().numpy()
                    if sum(b_len):
                        out = b.feature_distortion([(gen[s], nat[s], f, c, k) for s, (f, c, k) in enumerate(groups)], b_len,
                                                   path, path_len, mask, voiced_above).cpu().numpy()
                    else:
                        out = np.zeros((len(group), ns, 4))
                    for k, i in enumerate(group):
                        rows[i] = out[k]
                        info[i] = (ta[i], tb[i], pairs[k], status[k])
    if world > 1:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("evaluate_files with WORLD_SIZE > 1 needs torch.distributed to be initialised: the ranks' "
                               "rows have to be put together")
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        packed = torch.from_numpy(rows).to(dev)                      # a row is another rank's or zeros: the sum is exact
        counts = torch.from_numpy(info).to(dev)
        dist.all_reduce(packed)
        dist.all_reduce(counts)
        rows, info = packed.cpu().numpy(), counts.cpu().numpy()
    return W.pool_distortion(rows, kinds), rows, info


def evaluate_report(streams, pooled, rows, info, jobs, align):
    """(the JSON object of evaluate's --out, the lines of --per-utterance) from evaluate_files' results."""
    obj = {"align": align, "utterances": int(len(jobs)), "flagged": int(np.count_nonzero(info[:, 3])), "streams": {}}
    for (name, _), p in zip(streams, pooled):
        obj["streams"][name] = p
    lines = []
    for i, j in enumerate(jobs):
        cols = [j[0]] + [str(int(v)) for v in info[i]]
        for g, p in enumerate(W.pool_distortion(rows[i:i + 1], [p_["kind"] for p_ in pooled])):
            if p["kind"] == 0:
                cols += ["%.17g" % p["mean_db"], str(p["pairs"])]
            else:
                cols += ["%.17g" % p["rmse_cents"], "%.17g" % p["vuv_error_percent"], str(p["voiced_pairs"]), str(p["pairs"])]
        lines.append("\t".join(cols))
    return obj, lines


def _read_scp(path, n=4):
    with open(path) as f:
        rows = [ln.split() for ln in f if ln.strip() and not ln.startswith("#")]
    bad = [r for r in rows if len(r) != n]
    if bad:
        raise SystemExit("every line needs %s paths: %r" % ({4: "four"}.get(n, n), bad[0]))
    return [tuple(r) for r in rows]


def parse_stream(text):
    """`dim:msd:win0,win1,...` of the command line -> (dim, [window files], msd), e.g. 1:1:lf0.win1,lf0.win2,lf0.win3."""
    dim, msd, wins = text.split(":", 2)
    return int(dim), [w for w in wins.split(",") if w], msd not in ("0", "")


def parse_named_stream(text):
    """`name:dim:msd:win0,win1,...` -> (name, dim, [window files], msd): parse_stream behind the stream's name, which
    `generate` needs (mgc, lf0 and bap feed synthesis), e.g. lf0:1:1:lf0.win1,lf0.win2,lf0.win3."""
    name, rest = text.split(":", 1)
    if not name:
        raise ValueError("a stream needs a name: " + text)
    return (name,) + parse_stream(rest)


def generate_arguments(ap, a):
    """generate_files' keyword arguments from `generate`'s parsed command line (ap.error where the postfilter's own
    options are missing)."""
    post = None
    if a.postfilter == "mcp":
        post = ("mcp", a.beta, a.length)
    elif a.postfilter == "mspf":
        if not (a.gen_stats and a.nat_stats):
            ap.error("--postfilter mspf needs --gen-stats and --nat-stats")
        post = ("mspf", a.gen_stats, a.nat_stats, a.emphasis, a.mspf_frame_length, a.mspf_fft_length)
    elif a.postfilter == "gv":
        if not (a.gv_mean and a.gv_var):
            ap.error("--postfilter gv needs --gv-mean and --gv-var")
        post = ("gv", a.gv_mean, a.gv_var, {} if a.gv_max_iter is None else {"max_iter": a.gv_max_iter})
    if a.frame_shift < 1:
        ap.error("--frame-shift must be positive")
    return dict(config=a.config, frame_shift=a.frame_shift, model=a.model, spkr=a.spkr, streams=a.stream, fs=a.fs,
                frame_period=a.frame_period, fft_size=a.fft_size, alpha=a.alpha, postfilter=post, edge=a.edge,
                unvoiced_value=a.unvoiced_value, keep_dir=a.keep_dir, max_batch_frames=a.max_batch_frames, resume=a.resume,
                f0_scale=a.f0_scale, formant_ratio=a.formant_ratio)


def __getattr__(name):
    # the chain over the drivers above lives beside them (generate.py imports this module)
    if name in ("Generator", "generate_files"):
        from . import generate
        return getattr(generate, name)
    raise AttributeError(name)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m hts-train-world_amd.recipe", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("analysis", "synth"):
        p = sub.add_parser(name)
        p.add_argument("--scp", required=True, help="job list, four paths per line in the CLI's argument order")
        p.add_argument("--frame-period", type=float, default=5.0)
        p.add_argument("--fft-size", type=int, default=0 if name == "analysis" else None, required=name == "synth")
        p.add_argument("--spec-dim", type=int, default=0, help="0: uncompressed files")
        p.add_argument("--ap-dim", type=int, default=24)
        if name == "analysis":
            p.add_argument("--gather", action="store_true",
                           help="several ranks (torchrun): gather the features to rank 0, which writes every file")
            p.add_argument("--resume", action="store_true",
                           help="skip utterances whose three output files are already complete (a run that was cut short)")
            p.add_argument("--f0", choices=W.F0_ESTIMATORS, default="dio", help="the f0 estimator in front of the chain")
            p.add_argument("--no-refine", action="store_true", help="the estimator's contour as it is: no StoneMask behind it")
            p.add_argument("--f0-floor", type=float, default=71.0, help="lower end of the estimator's search range in Hz")
            p.add_argument("--f0-ceil", type=float, default=800.0, help="upper end of the estimator's search range in Hz")
        if name == "synth":
            p.add_argument("--fs", type=int, required=True)
    p = sub.add_parser("modify", help="test.cpp for a file list: analysis, F0 scaling and formant shift, synthesis")
    p.add_argument("--scp", required=True, help="job list: in.wav out.wav [f0_scale [formant_ratio]] per line")
    p.add_argument("--f0-scale", type=float, default=None, help="for the lines that give none (default: not done)")
    p.add_argument("--formant-ratio", type=float, default=None, help="for the lines that give none (default: not done)")
    p.add_argument("--frame-period", type=float, default=5.0)
    p.add_argument("--f0", choices=W.F0_ESTIMATORS, default="dio", help="the f0 estimator in front of the chain")
    p.add_argument("--f0-floor", type=float, default=71.0, help="lower end of the estimator's search range in Hz")
    p.add_argument("--f0-ceil", type=float, default=800.0, help="upper end of the estimator's search range in Hz")
    p.add_argument("--d4c-threshold", type=float, default=MODIFY_D4C_THRESHOLD, help="D4C's voicing threshold (test.cpp's)")
    p.add_argument("--resume", action="store_true", help="skip utterances whose output wav is already complete")
    p.add_argument("--max-batch-frames", type=int, default=MAX_BATCH_FRAMES)
    p = sub.add_parser("gen-param", help="gen_param: mlpg on every stream of a list of ffo files")
    p.add_argument("--scp", required=True, help="job list: the ffo file, then one output path per stream")
    p.add_argument("--stream", action="append", required=True, type=parse_stream, metavar="DIM:MSD:WIN0,WIN1,...",
                   help="one per stream in the row's order: dimension, 1 if a voicing column precedes it, window files")
    p.add_argument("--var", required=True, help="one float32 row of variances in the ffo layout")
    p.add_argument("--edge", type=int, default=0, help="0 taps beyond the ends dropped (SPTK), 1 clamped (window.pl)")
    p.add_argument("--unvoiced-value", type=float, default=-1.0e10)
    p.add_argument("--resume", action="store_true", help="skip utterances whose stream files are already complete")
    p = sub.add_parser("gv-pdf", help="gv.mean and gv.var from the one-vector files of gv-data")
    p.add_argument("--scp", required=True, help="one gv-data file per line")
    p.add_argument("--out-dir", required=True)
    p = sub.add_parser("gen-param-gv", help="gen-param with parameter generation considering global variance")
    p.add_argument("--scp", required=True, help="job list: the ffo file, then one output path per stream")
    p.add_argument("--stream", action="append", required=True, type=parse_stream, metavar="DIM:MSD:WIN0,WIN1,...",
                   help="one per stream in the row's order: dimension, 1 if a voicing column precedes it, window files")
    p.add_argument("--var", required=True, help="one float32 row of variances in the ffo layout")
    p.add_argument("--gv-mean", required=True, help="gv.mean of gv-pdf")
    p.add_argument("--gv-var", required=True, help="gv.var of gv-pdf")
    p.add_argument("--label-dir", default=None, help="where <base>.lab of every ffo file lies (with --silence)")
    p.add_argument("--silence", action="append", default=[], help="a label name in whose segments GV is off (NOSILGV)")
    p.add_argument("--frame-shift-s", type=float, default=0.005, help="seconds per frame of the labels")
    p.add_argument("--max-iter", type=int, default=None, help="MAXGVITER (50)")
    p.add_argument("--epsilon", type=float, default=None, help="GVEPSILON (1e-4)")
    p.add_argument("--step-init", type=float, default=None, help="STEPINIT (1)")
    p.add_argument("--step-inc", type=float, default=None, help="STEPINC (1.2)")
    p.add_argument("--step-dec", type=float, default=None, help="STEPDEC (0.5)")
    p.add_argument("--hmm-weight", type=float, default=None, help="HMMWEIGHT (1)")
    p.add_argument("--gv-weight", type=float, default=None, help="GVWEIGHT (1)")
    p.add_argument("--no-scale", action="store_true", help="start from mlpg's trajectory as it is")
    p.add_argument("--edge", type=int, default=0, help="0 taps beyond the ends dropped (SPTK), 1 clamped (window.pl)")
    p.add_argument("--unvoiced-value", type=float, default=-1.0e10)
    p.add_argument("--resume", action="store_true", help="skip utterances whose stream files are already complete")
    p = sub.add_parser("trj-eval", help="trajectory training's outputs and cost (DNNDefine.trajectory_cost) of a list of "
                       "ffo files")
    p.add_argument("--scp", required=True, help="job list: the model's ffo rows, the target ffo rows ('-' for none: no "
                   "cost), the file to write ('-' for none)")
    p.add_argument("--stream", action="append", required=True, type=parse_stream, metavar="DIM:MSD:WIN0,WIN1,...",
                   help="one per stream in the row's order: dimension, 1 if a voicing column precedes it, window files")
    p.add_argument("--var", required=True, help="one float32 row of variances in the ffo layout")
    p.add_argument("--gv-var", required=True, help="gv.var: one float32 row over the static columns of all streams")
    p.add_argument("--msd-weight", type=float, default=1.0)
    p.add_argument("--gv-weight", type=float, default=1.0e-6)
    p.add_argument("--resume", action="store_true", help="skip utterances whose output file is already complete")
    p = sub.add_parser("dnn-forward", help="DNNSynthesis.py frame by frame: the acoustic model's outputs for a list of ffi "
                       "files")
    p.add_argument("--scp", required=True, help="one `ffi` or one `ffi ffo` pair per line (with targets: the cost)")
    p.add_argument("--model", required=True, help="the .npz of training.AcousticModel.save")
    p.add_argument("--out-dir", required=True, help="<base>.<extension> and <base>.var are written here")
    p.add_argument("--extension", default="ffo")
    p.add_argument("--spkr", type=int, default=None, help="speaker index (default: the last, as DNNSynthesis.py)")
    p = sub.add_parser("dnn-train", help="DNNTraining.py (SD and SAT; frame by frame or trajectory training): trains the acoustic model on a list "
                       "of ffi / ffo pairs")
    p.add_argument("--scp", required=True, help="one `ffi ffo` pair per line, or `ffi ffo speaker-index`")
    p.add_argument("--model", required=True, help="the .npz to write")
    p.add_argument("--inputs", type=int, required=True, help="float32 values per ffi row")
    p.add_argument("--outputs", type=int, required=True, help="float32 values per ffo row")
    p.add_argument("--units", type=int, nargs="*", default=[], help="the hidden layers' widths")
    p.add_argument("--spkrs", type=int, default=1, help="number of speakers (more than one: SAT mode)")
    p.add_argument("--variance-dir", default=None, help="the directory of ffo.var (SAT: <dir>/<speaker index>/ffo.var)")
    p.add_argument("--hidden-activation", default="sigmoid", choices=W.ACTIVATIONS)
    p.add_argument("--output-activation", default="linear", choices=W.ACTIVATIONS)
    p.add_argument("--keep-prob", type=float, default=0.5)
    p.add_argument("--optimizer", default="adam", choices=OPTIMIZERS)
    p.add_argument("--learning-rate", type=float, default=0.001)
    p.add_argument("--batch-size", type=int, default=256)
    p.add_argument("--epochs", type=int, default=100)
    p.add_argument("--steps", type=int, default=None, help="instead of --epochs")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--log-interval", type=int, default=100)
    p.add_argument("--save-interval", type=int, default=0)
    p.add_argument("--restore", default=None, help="a .npz to continue from: steps, draws and dropout offsets go on from "
                   "its step count; with --updates tf1 the optimiser's state too")
    p.add_argument("--updates", default="torch", choices=("torch", "tf1"), help="torch: torch.optim's update rules; tf1: "
                   "TF 1.x's own, in one launch of the library's kernel, with the optimiser's state saved in the .npz")
    p.add_argument("--adapt", action="store_true", help="DNNTraining.py's ADAPT mode: needs --restore with a SAT model; the last "
                   "speaker's sd_weights row starts at the mean of the others and the si_ parameters stay")
    p.add_argument("--stream", action="append", default=None, type=parse_stream, metavar="DIM:MSD:WIN0,WIN1,...",
                   help="trajectory training (DNNTraining.py -w): one per stream in the row's order; minibatches are then "
                   "--batch-size utterances, and gv.var is read beside ffo.var")
    p.add_argument("--msd-weight", type=float, default=1.0)
    p.add_argument("--gv-weight", type=float, default=1.0e-6)
    p = sub.add_parser("postfilter", help="postfiltering_mcp: formant emphasis on a list of mgc files")
    p.add_argument("--scp", required=True, help="job list: the mgc file, then the p_mgc file to write")
    p.add_argument("--order", type=int, required=True, help="order of the mel-cepstra: a row holds order + 1 float32")
    p.add_argument("--alpha", type=float, required=True, help="frequency warping of the mgc stream")
    p.add_argument("--beta", type=float, default=1.4, help="the postfiltering coefficient (pf_mcp)")
    p.add_argument("--length", type=int, default=4096, help="bins of the energy sums (IMPLEN)")
    p.add_argument("--resume", action="store_true", help="skip utterances whose p_mgc file is already complete")
    p = sub.add_parser("mgc2mgc", help="SPTK's mgc2mgc on a list of float32 files: another alpha, gamma or order")
    p.add_argument("--scp", required=True, help="job list: the file to read, then the file to write")
    p.add_argument("-m", type=int, default=25, dest="order", help="order of the input: a row holds m + 1 float32")
    p.add_argument("-a", type=float, default=0.0, dest="alpha", help="alpha of the input")
    p.add_argument("-g", type=float, default=None, dest="gamma", help="gamma of the input")
    p.add_argument("-c", type=int, default=None, dest="c", help="gamma of the input = -1 / C")
    p.add_argument("-n", action="store_true", dest="normalized", help="the input is gain-normalized")
    p.add_argument("-u", action="store_true", dest="multiplied", help="the input is multiplied by gamma")
    p.add_argument("-M", type=int, default=25, dest="out_order", help="order of the output")
    p.add_argument("-A", type=float, default=0.0, dest="out_alpha", help="alpha of the output")
    p.add_argument("-G", type=float, default=None, dest="out_gamma", help="gamma of the output")
    p.add_argument("-C", type=int, default=None, dest="out_c", help="gamma of the output = -1 / C")
    p.add_argument("-N", action="store_true", dest="out_normalized", help="gain-normalized output")
    p.add_argument("-U", action="store_true", dest="out_multiplied", help="output multiplied by gamma")
    p.add_argument("--resume", action="store_true", help="skip utterances whose output file is already complete")
    for name, text in (("lsp2mgc", "lspcheck | lsp2lpc | mgc2mgc -n -u: MGC-LSP files to plain MGC (.c_mgc) files"),
                       ("postfilter-lsp", "postfiltering_lsp: the LSP postfilter on a list of MGC-LSP files (.p_mgc out)")):
        p = sub.add_parser(name, help=text)
        p.add_argument("--scp", required=True, help="job list: the MGC-LSP file to read, then the file to write")
        p.add_argument("--order", type=int, required=True, help="order of the rows: a row holds gain and order LSPs")
        p.add_argument("--alpha", type=float, required=True, help="frequency warping of the mgc stream")
        p.add_argument("--gamma", type=float, required=True, help="gamma of the mgc stream, -1 <= gamma < 0")
        p.add_argument("--log-gain", action="store_true", help="the gain is stored as its logarithm (LNGAIN)")
        p.add_argument("--resume", action="store_true", help="skip utterances whose output file is already complete")
        if name == "lsp2mgc":
            p.add_argument("--out-order", type=int, default=None, help="order of the output (default: the input's)")
            p.add_argument("--out-alpha", type=float, default=None, help="alpha of the output (default: the input's)")
            p.add_argument("--out-gamma", type=float, default=None, help="gamma of the output (default: the input's)")
        else:
            p.add_argument("--beta", type=float, default=0.7, help="the postfiltering coefficient (pf_lsp)")
            p.add_argument("--length", type=int, default=4096, help="samples of the energy sums (IMPLEN)")
            p.add_argument("--compensate", action="store_true", help="put the energy difference into the gain, which "
                           "the script as written does not")
    p = sub.add_parser("mgcep", help="x2x +sf | frame | window | mgcep at gamma 0: mel-cepstra of a list of raw or wav files")
    p.add_argument("--scp", required=True, help="job list: the .raw (int16) or wav file, then the mgc file to write")
    p.add_argument("--frame-length", type=int, default=1200, help="FRAMELEN")
    p.add_argument("--frame-shift", type=int, default=240, help="FRAMESHIFT")
    p.add_argument("--fft-length", type=int, default=2048, help="FFTLEN")
    p.add_argument("--window", type=int, default=1, help="WINDOWTYPE: 0 Blackman, 1 Hamming, 2 Hanning (5 rectangular)")
    p.add_argument("--normalize", type=int, default=1, help="NORMALIZE: 0 none, 1 power, 2 magnitude")
    p.add_argument("--alpha", type=float, default=0.55, help="FREQWARP")
    p.add_argument("--order", type=int, default=49, help="MGCORDER: a row holds order + 1 float32")
    p.add_argument("--eps", type=float, default=1.0e-8, help="mgcep -e: added to the periodogram")
    p.add_argument("--no-pipe-float32", action="store_true", help="keep the windowed samples in double (SPTK built with "
                   "DOUBLE), not rounded to float32 as the pipe between window and mgcep does")
    p.add_argument("--resume", action="store_true", help="skip utterances whose mgc file is already complete")
    p.add_argument("--max-batch-frames", type=int, default=MAX_BATCH_FRAMES)
    p = sub.add_parser("mlsa-synth", help="excite | dfs | mglsadf | x2x +fs -o: raw and wav files from lists of lf0 and mgc files")
    p.add_argument("--scp", required=True, help="job list: the lf0 file, the mgc file, then the raw and the wav file to write")
    p.add_argument("--lowpass", required=True, help="the taps of `dfs -b` on the pulse branch: what makefilter.pl prints "
                   "at flag 0, or a file that holds it")
    p.add_argument("--highpass", required=True, help="the same for the noise branch (makefilter.pl's flag 1)")
    p.add_argument("--fs", type=int, default=48000, help="SAMPFREQ: turns lf0 into a period in samples")
    p.add_argument("--frame-shift", type=int, default=240, help="FRAMESHIFT")
    p.add_argument("--alpha", type=float, default=0.55, help="FREQWARP")
    p.add_argument("--order", type=int, default=49, help="MGCORDER: a row holds order + 1 float32")
    p.add_argument("--pade-order", type=int, default=5, help="mglsadf -P, 1 to 7 (gen_wave passes 7: the rows of orders 6 "
                   "and 7 are the plain Pade approximant here, SPTK's own were not at hand)")
    p.add_argument("--no-pipe-float32", action="store_true", help="keep every value in double (SPTK built with DOUBLE), not "
                   "rounded to float32 at each pipe of the shell line")
    p.add_argument("--resume", action="store_true", help="skip utterances whose raw and wav files are already complete")
    p.add_argument("--max-batch-frames", type=int, default=MAX_BATCH_FRAMES)
    p.description = ("The int16 samples are the filter's output clipped to [-32768, 32767] and truncated toward zero: a "
                     "reading of `x2x +fs -o` that is unpinned, like the parity of the whole stage with SPTK.")
    for cmd in ("mspf-stats", "mspf"):
        p = sub.add_parser(cmd, help="make_mspf: statistics of the modulation spectra of a list of files" if cmd == "mspf-stats"
                           else "postfiltering_mspf: the modulation-spectrum postfilter on a list of mgc files")
        p.add_argument("--scp", required=True, help="job list: the feature file and its label file ('-' for none)"
                       if cmd == "mspf-stats" else "job list: the mgc file, then the p_mgc file to write")
        p.add_argument("--dim", type=int, required=True, help="float32 values per row")
        p.add_argument("--name", default="mgc", help="the statistics files are <name>_dim<d>.mean / .stdd")
        p.add_argument("--frame-length", type=int, default=25, help="mspfLength")
        p.add_argument("--fft-length", type=int, default=64, help="mspfFFTLen")
        if cmd == "mspf-stats":
            p.add_argument("--out-dir", required=True)
            p.add_argument("--silence", action="append", default=[], help="a label name to drop (may be repeated)")
            p.add_argument("--frame-shift", type=float, default=0.005, help="seconds per frame")
        else:
            p.add_argument("--gen-stats", required=True, help="directory of the generated parameters' statistics")
            p.add_argument("--nat-stats", required=True, help="directory of the natural parameters' statistics")
            p.add_argument("--emphasis", type=float, default=1.0, help="mspfe")
            p.add_argument("--resume", action="store_true", help="skip utterances whose p_mgc file is already complete")
    stream_help = "one per stream in the row's order: dimension, 1 if the stream has a voicing column, window files"
    p = sub.add_parser("ffo", help="the recipe's ffo stage: frame-by-frame training targets from the stream files")
    p.add_argument("--scp", required=True, help="job list: one feature file per stream, then the ffo file to write")
    p.add_argument("--stream", action="append", required=True, type=parse_stream, metavar="DIM:MSD:WIN0,WIN1,...",
                   help=stream_help)
    p.add_argument("--unvoiced-value", type=float, default=-1.0e10, help="what an unvoiced frame of an msd stream holds")
    p.add_argument("--resume", action="store_true", help="skip utterances whose ffo file is already complete")
    p = sub.add_parser("stats", help="the recipe's stats stage: ffo.var, <name>.var and gv.var of a list of ffo files")
    p.add_argument("--scp", required=True, help="one ffo file per line")
    p.add_argument("--stream", action="append", required=True, type=parse_stream, metavar="DIM:MSD:WIN0,WIN1,...",
                   help=stream_help)
    p.add_argument("--out-dir", required=True)
    p.add_argument("--name", action="append", default=[], help="a stream's name, in order (default: mgc lf0 bap vib)")
    p = sub.add_parser("gv-data", help="make_data_gv: the per-utterance variance vectors of GV training")
    p.add_argument("--scp", required=True, help="job list: one feature file per stream, the label file ('-' for none), "
                   "then the cmp file to write")
    p.add_argument("--stream", action="append", required=True, type=parse_stream, metavar="DIM:MSD:WIN0,WIN1,...",
                   help=stream_help + " (the windows may be left empty)")
    p.add_argument("--sampling-rate", type=int, required=True)
    p.add_argument("--frame-shift", type=int, required=True, help="samples per frame")
    p.add_argument("--silence", action="append", default=[], help="a label name to drop (may be repeated)")
    p.add_argument("--unvoiced-value", type=float, default=-1.0e10)
    p.add_argument("--resume", action="store_true", help="skip utterances whose cmp file is already complete")
    p = sub.add_parser("ffi", help="make_train_data_dnn / make_gen_data_dnn: the acoustic model's input rows from label files "
                       "(makefeature.pl | x2x +af)")
    p.add_argument("--scp", required=True, help="job list: the label file, then the ffi file to write")
    p.add_argument("--config", required=True, help="the question config (qconf)")
    p.add_argument("--frame-shift", type=int, required=True, help="one frame in the label's time unit of 100 ns (50000 for 5 ms)")
    p.add_argument("--resume", action="store_true", help="skip utterances whose ffi file is already complete")
    p = sub.add_parser("generate", help="aligned labels to wavs in one pass per batch: ffi, dnn-forward, gen-param, the "
                       "postfilter and synth without a file between them")
    p.add_argument("--scp", required=True, help="job list: the label file, then the wav to write")
    p.add_argument("--config", required=True, help="the question config (qconf)")
    p.add_argument("--frame-shift", type=int, required=True, help="one frame in the label's time unit of 100 ns (50000 for 5 ms)")
    p.add_argument("--model", required=True, help="the .npz of training.AcousticModel.save")
    p.add_argument("--spkr", type=int, default=None, help="speaker index (default: the last, as DNNSynthesis.py)")
    p.add_argument("--stream", action="append", required=True, type=parse_named_stream, metavar="NAME:DIM:MSD:WIN0,WIN1,...",
                   help="one per stream in the ffo row's order; mgc, lf0 and bap feed synthesis, any other is generated only")
    p.add_argument("--fs", type=int, required=True)
    p.add_argument("--frame-period", type=float, default=5.0)
    p.add_argument("--fft-size", type=int, required=True)
    p.add_argument("--alpha", type=float, required=True, help="frequency warping of the mgc stream (the mcp postfilter's)")
    p.add_argument("--postfilter", default="none", choices=("none", "mcp", "mspf", "gv"),
                   help="gv: gen-param-gv in gen-param's place and no postfilter after it")
    p.add_argument("--gv-mean", default=None, help="gv: gv.mean of gv-pdf")
    p.add_argument("--gv-var", default=None, help="gv: gv.var of gv-pdf")
    p.add_argument("--gv-max-iter", type=int, default=None, help="gv: MAXGVITER (50)")
    p.add_argument("--beta", type=float, default=1.4, help="mcp: the postfiltering coefficient (pf_mcp)")
    p.add_argument("--length", type=int, default=4096, help="mcp: bins of the energy sums (IMPLEN)")
    p.add_argument("--gen-stats", default=None, help="mspf: directory of the generated parameters' statistics")
    p.add_argument("--nat-stats", default=None, help="mspf: directory of the natural parameters' statistics")
    p.add_argument("--emphasis", type=float, default=1.0, help="mspf: mspfe")
    p.add_argument("--mspf-frame-length", type=int, default=25, help="mspf: mspfLength")
    p.add_argument("--mspf-fft-length", type=int, default=64, help="mspf: mspfFFTLen")
    p.add_argument("--edge", type=int, default=0, help="0 taps beyond the ends dropped (SPTK), 1 clamped (window.pl)")
    p.add_argument("--unvoiced-value", type=float, default=-1.0e10)
    p.add_argument("--keep-dir", default=None, help="also leave the staged commands' files here: <base>.ffi, .ffo, .var, "
                   "one file per stream and .p_mgc")
    p.add_argument("--resume", action="store_true", help="skip utterances whose wav is already complete")
    p.add_argument("--max-batch-frames", type=int, default=MAX_BATCH_FRAMES)
    p.add_argument("--f0-scale", type=float, default=None, help="multiply the generated f0 by this ahead of synthesis")
    p.add_argument("--formant-ratio", type=float, default=None, help="stretch the generated spectral envelope along the "
                   "frequency axis by this ahead of synthesis")
    p = sub.add_parser("evaluate", help="objective measures of generated against natural feature files: mel-cepstral "
                       "distortion, lf0 RMSE, V/UV error, along a DTW path or by truncation")
    p.add_argument("--scp", required=True, help="job list: per --stream in order the generated then the natural file, and the "
                   "natural utterance's label file last ('-' for none)")
    p.add_argument("--stream", action="append", required=True, type=parse_eval_stream, metavar="NAME:DIM",
                   help="mgc: cepstral distortion over columns 1 .. DIM-1; lf0: RMSE and V/UV error; any other name: cepstral "
                   "distortion over all columns")
    p.add_argument("--align", choices=("dtw", "truncate"), default="dtw", help="dtw: along the path found on the mgc stream")
    p.add_argument("--with-c0", action="store_true", help="score column 0 of mgc too")
    p.add_argument("--silence", action="append", default=[], help="a label name whose natural frames are left out (may be repeated)")
    p.add_argument("--frame-shift-s", type=float, default=0.005, help="seconds per frame, for the label files")
    p.add_argument("--voiced-above", type=float, default=-1.0e9, help="an lf0 value above this is voiced")
    p.add_argument("--out", default=None, help="the pooled figures and counts as one JSON object")
    p.add_argument("--per-utterance", default=None, help="a tab-separated line per utterance, in the job list's order")
    p.add_argument("--max-batch-frames", type=int, default=MAX_BATCH_FRAMES)
    a = ap.parse_args(argv)
    if a.cmd == "evaluate":
        import json
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:                # torchrun: the ranks' rows are put together
            import torch
            import torch.distributed as dist
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
            if not dist.is_initialized():
                dist.init_process_group(os.environ.get("WM_BACKEND", "nccl"))
        jobs = [r[:-1] + (None if r[-1] == "-" else r[-1],) for r in _read_scp(a.scp, 2 * len(a.stream) + 1)]
        try:
            pooled, rows, info = evaluate_files(jobs, a.stream, a.align, a.with_c0, a.silence, a.frame_shift_s,
                                                a.voiced_above, max_batch_frames=a.max_batch_frames)
        except ValueError as err:
            ap.error(str(err))
        obj, lines = evaluate_report(a.stream, pooled, rows, info, jobs, a.align)
        if _rank_world()[0] == 0:
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(obj, f, indent=1)
                    f.write("\n")
            if a.per_utterance:
                with open(a.per_utterance, "w") as f:
                    f.write("".join(ln + "\n" for ln in lines))
            print(json.dumps(obj))
        return 0
    if a.cmd == "modify":
        try:
            jobs = read_modify_list(a.scp, a.f0_scale, a.formant_ratio)
            n = modify_files(jobs, a.frame_period, a.f0, a.f0_floor, a.f0_ceil, a.d4c_threshold,
                             max_batch_frames=a.max_batch_frames, resume=a.resume)
        except ValueError as err:
            ap.error(str(err))
        print("complete. %d frames" % n)
        return 0
    if a.cmd == "generate":
        from . import generate
        n, flagged = generate.generate_files(_read_scp(a.scp, 2), **generate_arguments(ap, a))
        print("complete. %d frames, %d utterances flagged" % (n, len(flagged)))
        return 0
    if a.cmd == "ffi":
        if a.frame_shift < 1:
            ap.error("--frame-shift must be positive")
        n = ffi_files(_read_scp(a.scp, 2), a.config, a.frame_shift, resume=a.resume)
        print("complete. %d frames" % n)
        return 0
    if a.cmd == "ffo":
        n = ffo_files(_read_scp(a.scp, len(a.stream) + 1), a.stream, a.unvoiced_value, resume=a.resume)
        print("complete. %d frames" % n)
        return 0
    if a.cmd == "stats":
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:                # torchrun: the ranks' moments are gathered
            import torch
            import torch.distributed as dist
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
            if not dist.is_initialized():
                dist.init_process_group(os.environ.get("WM_BACKEND", "nccl"))
        n = stats_files([r[0] for r in _read_scp(a.scp, 1)], a.stream, a.out_dir, tuple(a.name) or ("mgc", "lf0", "bap", "vib"))
        print("complete. %d frames" % n)
        return 0
    if a.cmd == "gv-data":
        jobs = [r[:-2] + (None if r[-2] == "-" else r[-2], r[-1]) for r in _read_scp(a.scp, len(a.stream) + 2)]
        done = gv_data_files(jobs, a.stream, a.sampling_rate, a.frame_shift, a.silence, a.unvoiced_value, resume=a.resume)
        for path in done:
            print(path)
        return 0
    if a.cmd == "mspf-stats":
        jobs = [(f, None if lab == "-" else lab) for f, lab in _read_scp(a.scp, 2)]
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:                # torchrun: the ranks' sums are all-reduced
            import torch
            import torch.distributed as dist
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
            if not dist.is_initialized():
                dist.init_process_group(os.environ.get("WM_BACKEND", "nccl"))
        n = mspf_stats_files(jobs, a.dim, a.out_dir, a.name, a.silence, a.frame_shift, a.frame_length, a.fft_length)
        print("complete. %d frames" % n)
        return 0
    if a.cmd == "mspf":
        n = mspf_files(_read_scp(a.scp, 2), a.dim, a.gen_stats, a.nat_stats, a.name, a.emphasis, a.frame_length,
                       a.fft_length, resume=a.resume)
        print("complete. %d frames" % n)
        return 0
    if a.cmd == "mgcep":
        try:
            mgcep_check(a.frame_length, a.frame_shift, a.fft_length, a.window, a.normalize, a.alpha, a.order, a.eps,
                        a.max_batch_frames)
        except ValueError as err:
            ap.error(str(err))
        n, flagged = mgcep_files(_read_scp(a.scp, 2), a.frame_length, a.frame_shift, a.fft_length, a.window, a.normalize,
                                 a.alpha, a.order, a.eps, pipe_float32=not a.no_pipe_float32,
                                 max_batch_frames=a.max_batch_frames, resume=a.resume)
        print("complete. %d frames, %d utterances flagged" % (n, len(flagged)))
        return 0
    if a.cmd == "mlsa-synth":
        try:
            mlsa_synth_check(a.fs, a.frame_shift, a.order, a.alpha, a.pade_order, a.max_batch_frames)
            taps = read_taps(a.lowpass), read_taps(a.highpass)
        except ValueError as err:
            ap.error(str(err))
        n, flagged = mlsa_synth_files(_read_scp(a.scp, 4), taps[0], taps[1], a.fs, a.frame_shift, a.order, a.alpha,
                                      a.pade_order, pipe_float32=not a.no_pipe_float32,
                                      max_batch_frames=a.max_batch_frames, resume=a.resume)
        print("complete. %d frames, %d utterances flagged" % (n, len(flagged)))
        return 0
    if a.cmd == "mgc2mgc":
        n = mgc2mgc_files(_read_scp(a.scp, 2), a.order, a.alpha, sptk_gamma(a.gamma, a.c), a.out_order, a.out_alpha,
                          sptk_gamma(a.out_gamma, a.out_c), a.normalized, a.multiplied, a.out_normalized, a.out_multiplied,
                          resume=a.resume)
        print("complete. %d frames" % n)
        return 0
    if a.cmd in ("lsp2mgc", "postfilter-lsp"):
        try:
            if a.cmd == "lsp2mgc":
                lsp_check(a.order, a.alpha, a.gamma, a.out_order, a.out_alpha, a.out_gamma)
            else:
                lsp_check(a.order, a.alpha, a.gamma, beta=a.beta, length=a.length)
        except ValueError as err:
            ap.error(str(err))
        if a.cmd == "lsp2mgc":
            n = lsp2mgc_files(_read_scp(a.scp, 2), a.order, a.alpha, a.gamma, a.log_gain, a.out_order, a.out_alpha,
                              a.out_gamma, resume=a.resume)
        else:
            n = postfilter_lsp_files(_read_scp(a.scp, 2), a.order, a.alpha, a.gamma, a.beta, a.length, a.log_gain,
                                     a.compensate, resume=a.resume)
        print("complete. %d frames" % n)
        return 0
    if a.cmd == "postfilter":
        n = postfilter_files(_read_scp(a.scp, 2), a.order, a.alpha, a.beta, a.length, resume=a.resume)
        print("complete. %d frames" % n)
        return 0
    if a.cmd == "dnn-train":
        rows = []
        with open(a.scp) as f:
            for ln in f:
                w = ln.split()
                if w:
                    rows.append((w[0], w[1]) + ((int(w[2]),) if len(w) > 2 else ()))
        train_files(rows, a.model, a.inputs, a.units, a.outputs, a.spkrs, a.variance_dir, a.hidden_activation,
                    a.output_activation, a.keep_prob, a.optimizer, a.learning_rate, a.batch_size, a.epochs, a.steps, a.seed,
                    a.log_interval, a.save_interval, a.restore, a.stream, a.msd_weight, a.gv_weight, updates=a.updates,
                    adapt=a.adapt)
        return 0
    if a.cmd == "dnn-forward":
        forward_files(read_forward_scp(a.scp), a.model, a.out_dir, a.spkr, a.extension)
        return 0
    if a.cmd == "trj-eval":
        jobs = [(p_, None if o_ == "-" else o_, None if w_ == "-" else w_) for p_, o_, w_ in _read_scp(a.scp, 3)]
        costs = trajectory_files(jobs, a.stream, a.var, a.gv_var, a.msd_weight, a.gv_weight, resume=a.resume)
        for j, cost in zip(jobs, costs):
            if cost is not None:
                print("Evaluation: cost = %e (%s)" % (cost, j[0]))
        return 0
    if a.cmd == "gv-pdf":
        print("complete. %d files" % gv_pdf_files([r[0] for r in _read_scp(a.scp, 1)], a.out_dir))
        return 0
    if a.cmd == "gen-param-gv":
        opts = {k: getattr(a, k) for k in GV_OPTIONS[:-1] if getattr(a, k) is not None}
        if a.no_scale:
            opts["scale"] = 0
        n = gen_param_gv_files(_read_scp(a.scp, 1 + len(a.stream)), a.stream, a.var, a.gv_mean, a.gv_var, a.label_dir,
                               a.silence, a.frame_shift_s, a.edge, a.unvoiced_value, resume=a.resume, **opts)
        print("complete. %d frames" % n)
        return 0
    if a.cmd == "gen-param":
        n = gen_param_files(_read_scp(a.scp, 1 + len(a.stream)), a.stream, a.var, a.edge, a.unvoiced_value,
                            resume=a.resume)
        print("complete. %d frames" % n)
        return 0
    jobs = _read_scp(a.scp)
    if a.cmd == "analysis":
        if a.gather and int(os.environ.get("WORLD_SIZE", "1")) > 1:
            import torch
            import torch.distributed as dist
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
            dist.init_process_group(os.environ.get("WM_BACKEND", "nccl"))
        n = analysis_files(jobs, a.frame_period, a.fft_size, a.spec_dim, a.ap_dim, gather=a.gather, resume=a.resume,
                           f0_estimator=a.f0, refine=not a.no_refine, f0_floor=a.f0_floor, f0_ceil=a.f0_ceil)
    else:
        n = synth_files(jobs, a.frame_period, a.fft_size, a.fs, a.spec_dim, a.ap_dim)
    print("complete. %d frames" % n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
