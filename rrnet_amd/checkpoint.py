"""Full-state checkpoints: everything the next train_step reads, taken between two optimizer steps without stopping
the loop, written by a thread, and the way back in.

The state: FlatParams.flat, FlatAdam.exp_avg / exp_avg_sq / step_count, the learning rate and the scheduler's
state_dict, every module buffer by name (BatchNorm running statistics; num_batches_tracked as int64), the step index,
the training loader's position, and a fingerprint of the flat buffer's layout.  Random-number-generator states are not
part of it: no kernel of the step consumes a random number, and the loaders draw from (seed, rank, epoch, index).
With the guarded optimiser step on two optional entries join it: `ema`, the averaged weights, a fourth flat
buffer handled like the other three, and `guard`, the step's control record; a file taken without them is unchanged, and
extras_plan() says what a load does with each combination of file and live optimiser.

Taking it (StateWriter.save_state, on the training stream): join the auxiliary streams, three rr_state_snapshot launches
(copy + digest in one pass) into device staging buffers, the buffers packed into staging tensors, one event.  A copy
stream waits for the event and moves staging and digests into pinned host memory; one worker thread waits for that copy,
refuses a state holding a NaN or an Inf, writes `state-{step}.pth.tmp`, fsyncs, renames, and prunes old files.  The
training thread never reads the device for any of this.

`save_ckp` (the reference's weights-only file) is untouched; these files live beside it."""
import copy
import glob
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

FORMAT_VERSION = 1
CHUNK = 65536                      # elements per digest record
FLAT_NAMES = ("flat", "exp_avg", "exp_avg_sq")
_STATE_RE = re.compile(r"^state-(\d+)\.pth$")


class StateError(RuntimeError):
    """A state file that cannot be trusted or does not fit the live model."""


# ---------------------------------------------------------------------------------------------------------------------
# host-side pieces (no device needed)
# ---------------------------------------------------------------------------------------------------------------------
def digest_reference(words, chunk=CHUNK):
    """The digest of include/rrnet_hip.h (rr_state_snapshot) in numpy: `words` are the uint32 bit patterns (a float32
    array is reinterpreted) -> uint64 [ceil(n / chunk), 3] with wrap-around sums."""
    u = np.ascontiguousarray(words)
    if u.dtype != np.uint32:
        u = u.view(np.uint32)
    u = u.reshape(-1).astype(np.uint64)
    n = u.size
    nchunks = (n + chunk - 1) // chunk
    out = np.zeros((nchunks, 3), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for c in range(nchunks):
            part = u[c * chunk:(c + 1) * chunk]
            j1 = np.arange(1, part.size + 1, dtype=np.uint64)
            out[c, 0] = part.sum(dtype=np.uint64)
            out[c, 1] = (j1 * part).sum(dtype=np.uint64)
            out[c, 2] = np.count_nonzero((part & np.uint64(0x7f800000)) == np.uint64(0x7f800000))
    return out


def list_states(log_dir):
    """[(step, path)] of the `state-<step>.pth` files in `log_dir`, newest (highest step) first; `*.tmp` are ignored."""
    found = []
    for p in glob.glob(os.path.join(log_dir, "state-*.pth")):
        m = _STATE_RE.match(os.path.basename(p))
        if m:
            found.append((int(m.group(1)), p))
    return sorted(found, reverse=True)


def latest_state(log_dir):
    """Path of the highest-numbered `state-*.pth` in `log_dir`, or None."""
    states = list_states(log_dir)
    return states[0][1] if states else None


def layout_fingerprint(module, fp):
    """What a flat buffer's contents mean: the ordered (parameter name, shape, flat offset) list, the buffer's length
    and the model class.  The physical layout (OHWI filters, 16-byte padding) is private to FlatParams; two models
    with equal fingerprints place every weight at the same word."""
    names = {id(p): n for n, p in module.named_parameters()}
    return {"model": type(module).__name__, "numel": int(fp.numel),
            "entries": [(names.get(id(p), "?"), tuple(int(s) for s in p.shape), int(fp._offs[id(p)])) for p in fp.params]}


def compare_fingerprint(saved, live):
    """Raises StateError naming the first entry in which the saved layout differs from the live one."""
    if saved["model"] != live["model"]:
        raise StateError("state was saved from a %s, the live model is a %s" % (saved["model"], live["model"]))
    for i, (s, l) in enumerate(zip(saved["entries"], live["entries"])):
        s, l = (s[0], tuple(s[1]), s[2]), (l[0], tuple(l[1]), l[2])
        if s != l:
            raise StateError("flat layout differs at parameter #%d: saved %s %s at offset %d, live %s %s at offset %d"
                             % (i, s[0], s[1], s[2], l[0], l[1], l[2]))
    if len(saved["entries"]) != len(live["entries"]):
        i = min(len(saved["entries"]), len(live["entries"]))
        longer, which = (saved, "saved") if len(saved["entries"]) > i else (live, "live")
        raise StateError("flat layout differs at parameter #%d: only the %s model has %s %s (%d vs %d parameters)"
                         % (i, which, longer["entries"][i][0], tuple(longer["entries"][i][1]), len(saved["entries"]),
                            len(live["entries"])))
    if saved["numel"] != live["numel"]:
        raise StateError("flat buffer length differs: saved %d, live %d" % (saved["numel"], live["numel"]))


def state_names(optimizer):
    """The flat buffers a state of this optimiser holds, in digest order: FLAT_NAMES, and `ema` behind them when the
    optimiser keeps averaged weights (FlatAdam(ema_decay=...)).  Without the option the list, and with it the file, is
    the one of format 1 as it always was."""
    return FLAT_NAMES + (("ema",) if getattr(optimizer, "ema", None) is not None else ())


def guard_ctl_from_step_count(step_count, beta1, beta2):
    """The guard's control record (float64, ops.GUARD_CTL_WORDS) for an optimiser that took `step_count` unguarded steps:
    applied = step_count, the two running products by step_count host multiplications (what the device would have done
    one step at a time), every other counter 0.  The per-step slots are rewritten by the next decide launch."""
    from rrnet_amd import ops
    ctl = ops.guard_ctl_fresh().numpy().copy()
    b1p = b2p = 1.0
    for _ in range(int(step_count)):
        b1p *= float(beta1)
        b2p *= float(beta2)
    ctl[0], ctl[3], ctl[4] = float(int(step_count)), b1p, b2p
    return ctl


def extras_plan(sd, optimizer):
    """What load_state does with the two optional entries of a state file, decided on the host from the file's keys and
    the live optimiser's options -> (ema, guard):
      ema:   'restore' (file has it, EMA on: verify its digest, copy it in), 'init' (file lacks it, EMA on: start the
             average from the loaded weights, with a warning), 'ignore' (file has it, EMA off: a note), None;
      guard: 'restore' (file has it, a guard is on), 'derive' (file lacks it, a guard is on: guard_ctl_from_step_count),
             None (no guard on; an entry in the file is not needed)."""
    has_ema, want_ema = "ema" in sd, getattr(optimizer, "ema", None) is not None
    ema = ("restore" if has_ema else "init") if want_ema else ("ignore" if has_ema else None)
    guard = None
    if getattr(optimizer, "ctl", None) is not None:
        guard = "restore" if "guard" in sd else "derive"
    return ema, guard


def _buffer_index(module):
    """Buffers grouped by dtype: {dtype name: [(buffer name, shape, offset into that dtype's packed tensor)]}, and the
    packed lengths."""
    index, sizes = {}, {}
    for name, b in module.named_buffers():
        if b.numel() == 0:
            continue
        key = str(b.dtype).replace("torch.", "")
        off = sizes.get(key, 0)
        index.setdefault(key, []).append((name, tuple(int(s) for s in b.shape), off))
        sizes[key] = off + b.numel()
    return index, sizes


def _compare_buffers(saved, live):
    for key in sorted(set(saved) | set(live)):
        s, l = saved.get(key, []), live.get(key, [])
        for i, (a, b) in enumerate(zip(s, l)):
            a, b = (a[0], tuple(a[1]), a[2]), (b[0], tuple(b[1]), b[2])
            if a != b:
                raise StateError("module buffers (%s) differ at #%d: saved %s %s, live %s %s" % (key, i, a[0], a[1], b[0], b[1]))
        if len(s) != len(l):
            raise StateError("module buffers (%s) differ: saved %d, live %d" % (key, len(s), len(l)))


# ---------------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------------
class StateWriter:
    """save_state(step) enqueues a consistent copy of the training state on the current stream and returns; a copy
    stream and one worker thread turn it into `<log_dir>/state-{step}.pth`.  Staging (device: 3 x numel floats; host:
    the same, pinned) is allocated once, at the first save, so a second save first waits for the one in flight.  An
    exception in the thread is re-raised by the next save_state or by close(); a refusal (NaN / Inf in the state) is
    printed there as a warning and kept in `warnings`."""

    def __init__(self, module, optimizer, log_dir, lr_sch=None, loader=None, keep=2, chunk=CHUNK):
        self.module, self.opt, self.fp = module, optimizer, optimizer.fp
        self.lr_sch, self.loader = lr_sch, loader
        self.log_dir, self.keep, self.chunk = log_dir, max(int(keep), 1), int(chunk)
        self.device = self.fp.flat.device
        self.warnings = []
        self._reported = 0
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="rr-state")
        self._job = None
        self._staged = False

    def _sources(self):
        src = (self.fp.flat, self.opt.exp_avg, self.opt.exp_avg_sq)
        return src + ((self.opt.ema,) if len(self.names) > len(FLAT_NAMES) else ())

    def _allocate(self):
        n = self.fp.numel
        nchunks = (n + self.chunk - 1) // self.chunk
        self.names = state_names(self.opt)                # the averaged weights are a fourth source when they exist
        self.d_stage = [torch.empty(n, dtype=torch.float32, device=self.device) for _ in self.names]
        self.d_digest = torch.empty((len(self.names), nchunks, 3), dtype=torch.int64, device=self.device)
        self.h_stage = [torch.empty(n, dtype=torch.float32).pin_memory() for _ in self.names]
        self.h_digest = torch.empty((len(self.names), nchunks, 3), dtype=torch.int64).pin_memory()
        self.d_guard = self.h_guard = None                # the guard's control record, when a guard is on
        if getattr(self.opt, "ctl", None) is not None:
            self.d_guard = torch.empty_like(self.opt.ctl)
            self.h_guard = torch.empty(self.opt.ctl.shape, dtype=torch.float64).pin_memory()
        self.buf_index, sizes = _buffer_index(self.module)
        self.d_bufs = {k: torch.empty(sz, dtype=getattr(torch, k), device=self.device) for k, sz in sizes.items()}
        self.h_bufs = {k: torch.empty(sz, dtype=getattr(torch, k)).pin_memory() for k, sz in sizes.items()}
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.fingerprint = layout_fingerprint(self.module, self.fp)
        self._staged = True

    def _collect(self):
        """Waits for the save in flight; re-raises what its thread raised; prints refusals not yet reported."""
        job, self._job = self._job, None
        try:
            if job is not None:
                job.result()
        finally:
            for w in self.warnings[self._reported:]:
                print("warning: " + w, flush=True)
            self._reported = len(self.warnings)

    @torch.no_grad()
    def save_state(self, step):
        from rrnet_amd import ops
        self._collect()                                   # the staging buffers are single
        if not self._staged:
            self._allocate()
        cur = torch.cuda.current_stream(self.device)
        ops.join_aux_streams(self.device)                 # weight gradients / Adam's producers on their side streams
        for i, src in enumerate(self._sources()):
            ops.state_snapshot(src, self.d_stage[i], self.chunk, out=self.d_digest[i])
        if self.d_guard is not None:
            self.d_guard.copy_(self.opt.ctl)               # on the training stream, behind the step that wrote it
        bufs = dict(self.module.named_buffers())
        for k, rows in self.buf_index.items():            # one gather per dtype into its packed staging tensor
            torch.cat([bufs[name].detach().reshape(-1) for name, _, _ in rows], out=self.d_bufs[k])
        taken = torch.cuda.Event()
        taken.record(cur)
        # everything below reads host values only
        meta = {"format": FORMAT_VERSION, "step": int(step), "step_count": int(self.opt.step_count),
                "lr": float(self.opt.param_groups[0]["lr"]),
                "lr_sch": copy.deepcopy(self.lr_sch.state_dict()) if self.lr_sch is not None else None,
                "loader_position": int(self.loader.position()) if self.loader is not None else None,
                "fingerprint": self.fingerprint, "buffer_index": self.buf_index, "chunk": self.chunk}
        self.copy_stream.wait_event(taken)
        with torch.cuda.stream(self.copy_stream):
            for h, d in zip(self.h_stage, self.d_stage):
                h.copy_(d, non_blocking=True)
            self.h_digest.copy_(self.d_digest, non_blocking=True)
            if self.d_guard is not None:
                self.h_guard.copy_(self.d_guard, non_blocking=True)
            for k in self.d_bufs:
                self.h_bufs[k].copy_(self.d_bufs[k], non_blocking=True)
            landed = torch.cuda.Event()
            landed.record(self.copy_stream)
        # the next kernels of the training stream may overwrite the LIVE buffers at once (the copies read staging); the next
        # save_state overwrites staging only after _collect() has seen this job finish, i.e. after `landed`
        self._job = self._pool.submit(self._write, meta, landed)

    def _write(self, meta, landed):
        landed.synchronize()
        bad = self.h_digest[:, :, 2].sum(dim=1).tolist()
        if any(bad):
            self.warnings.append("state of step %d not written: %s; the previous state file stays"
                                 % (meta["step"], ", ".join("%s holds %d NaN/Inf" % (n, c) for n, c in zip(self.names, bad) if c)))
            return None
        obj = dict(meta)
        for name, h in zip(self.names, self.h_stage):
            obj[name] = h
        if self.h_guard is not None:
            obj["guard"] = self.h_guard
        obj["digests"] = self.h_digest
        obj["buffers"] = dict(self.h_bufs)
        os.makedirs(self.log_dir, exist_ok=True)
        path = os.path.join(self.log_dir, "state-%d.pth" % meta["step"])
        tmp = path + ".tmp"
        with open(tmp, "wb") as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
        # the file just written and the newest keep - 1 older ones stay; a file with a HIGHER number (a damaged one that
        # resume='auto' passed over) is not counted, or it would push the new file out
        older = [p for s, p in list_states(self.log_dir) if s < meta["step"]]
        for old in older[self.keep - 1:]:
            os.remove(old)
        return path

    def close(self):
        """Waits for the save in flight and stops the thread; re-raises / reports like save_state."""
        try:
            self._collect()
        finally:
            self._pool.shutdown(wait=True)


# ---------------------------------------------------------------------------------------------------------------------
# the way back in
# ---------------------------------------------------------------------------------------------------------------------
def _same_digest(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


@torch.no_grad()
def load_state(path, module, optimizer, lr_sch=None, loader=None):
    """Loads `path` into the live module / optimizer / scheduler / loader and returns the step to continue at (the
    saved step + 1).  Nothing live is touched before the file's version, its layout fingerprint and the digests of
    its three flat buffers (recomputed on the device from what was uploaded) have been checked; the digests are checked
    again on the live buffers after the copy."""
    from rrnet_amd import ops
    fp = optimizer.fp
    dev = fp.flat.device
    try:
        sd = torch.load(path, map_location="cpu", weights_only=False)
    except Exception as e:          # a torn or damaged file shows up as any of zip / pickle / storage errors
        raise StateError("%s cannot be read: %s: %s" % (path, type(e).__name__, e))
    if not isinstance(sd, dict) or sd.get("format") != FORMAT_VERSION:
        raise StateError("%s: format version %r, this code reads %d"
                         % (path, sd.get("format") if isinstance(sd, dict) else None, FORMAT_VERSION))
    compare_fingerprint(sd["fingerprint"], layout_fingerprint(module, fp))
    live_index, _ = _buffer_index(module)
    _compare_buffers(sd["buffer_index"], live_index)
    chunk = int(sd["chunk"])
    stored = sd["digests"]
    live = (fp.flat, optimizer.exp_avg, optimizer.exp_avg_sq)
    names = FLAT_NAMES
    ema_plan, guard_plan = extras_plan(sd, optimizer)
    if ema_plan == "restore":       # a fourth flat buffer, checked and copied like the other three
        live, names = live + (optimizer.ema,), names + ("ema",)
        if stored.shape[0] < len(names):
            raise StateError("%s: holds ema but no digest of it" % path)
    if guard_plan == "restore":
        g = sd["guard"]
        if not torch.is_tensor(g) or g.dtype != torch.float64 or g.numel() != optimizer.ctl.numel():
            raise StateError("%s: guard record has %s, the live one %d float64 words"
                             % (path, "%d %s words" % (g.numel(), g.dtype) if torch.is_tensor(g) else type(g).__name__,
                                optimizer.ctl.numel()))
    uploaded = []
    for i, name in enumerate(names):
        t = sd[name]
        if t.dtype != torch.float32 or t.numel() != fp.numel:
            raise StateError("%s: %s has %d %s words, the live buffer %d float32" % (path, name, t.numel(), t.dtype, fp.numel))
        u = t.to(dev)
        if not _same_digest(ops.state_snapshot(u, None, chunk).cpu(), stored[i]):
            raise StateError("%s: digest of %s does not match the stored one (damaged file or upload)" % (path, name))
        uploaded.append(u)
    for i, (dst, u) in enumerate(zip(live, uploaded)):
        dst.copy_(u)                                      # in place: the version counters move
        if not _same_digest(ops.state_snapshot(dst, None, chunk).cpu(), stored[i]):
            raise StateError("%s: digest of the live %s differs after the copy" % (path, names[i]))
    del uploaded
    fp.invalidate_wt()              # flipped-filter cache, bf16 filter copies, split-operand filter maxima
    optimizer.step_count = int(sd["step_count"])
    if ema_plan == "init":
        optimizer.ema.copy_(fp.flat)
        print("warning: %s holds no averaged weights: the average starts from the loaded weights" % path, flush=True)
    elif ema_plan == "ignore":
        print("note: %s holds averaged weights; the optimiser keeps none (ema_decay is not set), they are not loaded" % path,
              flush=True)
    if guard_plan == "restore":
        optimizer.ctl.copy_(sd["guard"].reshape(optimizer.ctl.shape))
    elif guard_plan == "derive":    # a state taken without a guard: Adam's bias correction continues from its step count
        b1, b2 = optimizer.param_groups[0]["betas"]
        optimizer.ctl.copy_(torch.from_numpy(guard_ctl_from_step_count(optimizer.step_count, b1, b2)))
    optimizer.param_groups[0]["lr"] = float(sd["lr"])
    if lr_sch is not None and sd["lr_sch"] is not None:
        lr_sch.load_state_dict(sd["lr_sch"])
    bufs = dict(module.named_buffers())
    for key, rows in sd["buffer_index"].items():
        packed = sd["buffers"][key].to(dev)
        for name, shape, off in rows:
            b = bufs[name]
            b.copy_(packed[off:off + b.numel()].view(b.shape))
    if loader is not None and sd["loader_position"] is not None:
        loader.seek(int(sd["loader_position"]))
    return int(sd["step"]) + 1


def resume(where, log_dir, module, optimizer, lr_sch=None, loader=None):
    """cfg.Train.resume: 'auto' tries the state files of `log_dir` from the newest down, reports each one that fails to
    load or to verify, and starts at step 0 when none is left; anything else is a path that must load.  Returns the step
    to start at."""
    if where != "auto":
        start = load_state(where, module, optimizer, lr_sch, loader)
        print("=> resumed from %s: continuing at step %d" % (where, start), flush=True)
        return start
    for _, path in list_states(log_dir):
        try:
            start = load_state(path, module, optimizer, lr_sch, loader)
        except StateError as e:
            print("warning: %s; trying the next older state" % e, flush=True)
            continue
        print("=> resumed from %s: continuing at step %d" % (path, start), flush=True)
        return start
    print("=> no usable state file in %s: starting at step 0" % log_dir, flush=True)
    return 0
