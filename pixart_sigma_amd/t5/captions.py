"""Caption strings to caption features inside the training step: reference train_scripts/train.py:161-168 (load_t5_feat = False),

    txt_tokens = tokenizer(batch[1], max_length=max_length, padding="max_length", truncation=True, return_tensors="pt")
    y = text_encoder(txt_tokens.input_ids, attention_mask=txt_tokens.attention_mask)[0][:, None];  y_mask = txt_tokens.attention_mask

CaptionEncoder.encode(list of str) -> (y fp32 (B, 1, L, 4096) on the device, mask int64 (B, L) on the HOST).  The calling process tokenises, so the mask
never visits the device and the denoiser's per-sample caption lengths cost no synchronisation.

The T5 encoder must compute on bf16 operands (trained T5-XXL activations overflow fp16; the reference loads it with torch_dtype=bfloat16), the PixArt-Sigma
configs train the denoiser on fp16 operands, and the operand type is one library per process.  So:

  * in a process of the bf16 build, T5Encoder runs in this process;
  * in a process of the f16 build, it runs in a WORKER: one fresh child process per CaptionEncoder (one per rank), started with subprocess and
    PXA_OPERAND_DTYPE=bf16 - never by replacing the program of a running process.  The worker loads the encoder once and serves requests: ids and masks go in
    and bf16 features come back through one multiprocessing.shared_memory block with two feature slots, used in turn, so the worker can fill one while
    the parent uploads the other (submit / collect; encode is the two in a row).  The parent uploads the features and widens them to fp32.

Worker rules.  Every wait on the worker has a time limit (start_timeout for loading the weights, timeout per request).  A worker that dies, or misses a limit,
raises CaptionWorkerError in the parent with the tail of the worker's stderr; it is never restarted and a request is never retried.  The parent terminates
and reaps the worker in close(), on garbage collection, at interpreter exit and on every error path.

Process count: the worker is a second process with the GPU open, so a rank is 2 GPU processes and a node of world size 8 runs 16 - which is the limit of
processes that may hold the GPUs open at once where this project runs.  Do not add a further GPU process per rank next to a CaptionEncoder worker.

Caption cleaning (the reference's ftfy / bs4 clean_caption, which train.py does not apply either) stays outside."""
import json
import os
import select
import subprocess
import sys
import tempfile
import time
import weakref

import torch

from .. import lib

TAG = "PXA-CAPTION"
STDERR_TAIL = 4000


class CaptionWorkerError(RuntimeError):
    pass


def tokenize(tokenizer, texts, max_length):
    """(ids, mask) int64 (B, max_length) on the host: the tokenizer call of reference train.py:163-165 (any callable with that signature)."""
    tok = tokenizer(list(texts), max_length=max_length, padding="max_length", truncation=True, return_tensors="pt")
    ids = torch.as_tensor(tok["input_ids"])[:, :max_length].to(torch.int64).cpu()
    mask = torch.as_tensor(tok["attention_mask"])[:, :max_length].to(torch.int64).cpu()
    return ids, mask


def _shm_layout(max_batch, L, d_model):
    """Byte offsets of (ids int32, mask int32, feature slot 0, feature slot 1) and the block's size; every offset a multiple of 64."""
    n_tok = (max_batch * L * 4 + 63) // 64 * 64
    n_feat = (max_batch * L * d_model * 2 + 63) // 64 * 64
    return (0, n_tok, 2 * n_tok, 2 * n_tok + n_feat), 2 * n_tok + 2 * n_feat


def _stop(proc, shm, errfile):
    """Terminate and reap the worker, drop the shared block.  Safe to call more than once."""
    if proc is not None and proc.poll() is None:
        try:
            proc.stdin.close()                       # the worker's request loop ends at end of input
        except OSError:
            pass
        try:
            proc.wait(timeout=0.2)
        except subprocess.TimeoutExpired:
            proc.terminate()
            try:
                proc.wait(timeout=10)
            except subprocess.TimeoutExpired:
                proc.kill()
                proc.wait()
    if proc is not None:
        for f in (proc.stdin, proc.stdout):
            try:
                f.close()
            except OSError:
                pass
    if shm is not None:
        for drop in (shm.close, shm.unlink):
            try:
                drop()
            except (OSError, BufferError):
                pass
    if errfile is not None:
        errfile.close()


class _Worker:
    """The child process of the f16 build's CaptionEncoder and the parent's end of its protocol.  Requests are lines on the child's stdin
    ("<TAG> <slot> <B>"), answers lines on its stdout ("<TAG> ok <slot>"); everything else the child prints is ignored."""

    def __init__(self, t5_path, L, device_index, max_batch, timeout, start_timeout, weight_dtype=None):
        from multiprocessing import shared_memory
        with open(os.path.join(t5_path, "config.json")) as f:
            self.d_model = int(json.load(f).get("d_model", 4096))
        self.L, self.max_batch, self.timeout = L, max_batch, timeout
        self.offsets, size = _shm_layout(max_batch, L, self.d_model)
        self.shm = shared_memory.SharedMemory(create=True, size=size)
        self.errfile = tempfile.TemporaryFile()
        env = dict(os.environ, PXA_OPERAND_DTYPE="bf16")
        env.pop("PXA_LIB_PATH", None)
        root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "") if env.get("PYTHONPATH") else root
        self.proc = subprocess.Popen([sys.executable, "-m", "pixart_sigma_amd.t5.captions", "--worker", "--t5-path", t5_path, "--shm", self.shm.name,
                                      "--length", str(L), "--max-batch", str(max_batch), "--device", str(device_index)] + (["--weight-dtype", weight_dtype] if weight_dtype else []),
                                     stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=self.errfile, env=env, cwd=root)
        self._finalizer = weakref.finalize(self, _stop, self.proc, self.shm, self.errfile)
        self._buf = b""
        self.pending = []                            # slots submitted and not collected, oldest first
        self.next_slot = 0
        self.failed = None
        self._await("ready", start_timeout)

    # ---- failure and shutdown
    def close(self):
        self._finalizer()

    @property
    def alive(self):
        return self.proc.poll() is None

    def _fail(self, what):
        tail = ""
        try:
            self.errfile.seek(0, os.SEEK_END)
            n = self.errfile.tell()
            self.errfile.seek(max(0, n - STDERR_TAIL))
            tail = self.errfile.read().decode(errors="replace")
        except (OSError, ValueError):
            pass
        rc = self.proc.poll()
        self.close()
        self.failed = f"caption worker: {what} (exit status {rc if rc is not None else 'none: it was still running and has been terminated'}); it is not " \
                      f"restarted.  Its stderr ends:\n{tail}"
        raise CaptionWorkerError(self.failed)

    def _await(self, word, limit):
        """Block until the worker's next protocol line, at most `limit` seconds; the line must be '<TAG> <word> ...'."""
        deadline = time.monotonic() + limit
        fd = self.proc.stdout.fileno()
        while True:
            while b"\n" in self._buf:
                line, self._buf = self._buf.split(b"\n", 1)
                parts = line.decode(errors="replace").split()
                if parts[:1] != [TAG]:
                    continue
                if parts[1:2] != [word]:
                    self._fail(f"answered {' '.join(parts[1:])!r} where {word!r} was expected")
                return parts[2:]
            left = deadline - time.monotonic()
            ready = select.select([fd], [], [], max(left, 0.0))[0] if left > 0 else []
            if not ready:
                self._fail(f"no {word!r} within its time limit of {limit:g} s")
            chunk = os.read(fd, 65536)
            if not chunk:
                try:
                    self.proc.wait(timeout=10)                       # end of its output: take the exit status for the message
                except subprocess.TimeoutExpired:
                    pass
                self._fail(f"died before answering {word!r}")
            self._buf += chunk

    # ---- requests
    def _view(self, which, dtype, count):
        return torch.frombuffer(self.shm.buf, dtype=dtype, count=count, offset=self.offsets[which])

    def submit(self, ids, mask):
        if self.failed:
            raise CaptionWorkerError(self.failed)
        B = ids.shape[0]
        if B > self.max_batch or ids.shape[1] != self.L:
            raise ValueError(f"caption worker was started for up to {self.max_batch} captions of {self.L} tokens, got {tuple(ids.shape)}")
        if len(self.pending) == 2:
            raise RuntimeError("caption worker: two requests are in flight already (two feature slots): collect one first")
        if self.pending:                             # the ids / mask area is shared by both slots: the worker must have read the previous request
            self._finish_oldest()
        slot, self.next_slot = self.next_slot, 1 - self.next_slot
        self._view(0, torch.int32, B * self.L).copy_(ids.reshape(-1))
        self._view(1, torch.int32, B * self.L).copy_(mask.reshape(-1))
        try:
            self.proc.stdin.write(f"{TAG} {slot} {B}\n".encode())
            self.proc.stdin.flush()
        except OSError:
            self._fail("died (its request pipe is closed)")
        self.pending.append([slot, B, False])
        return slot

    def _finish_oldest(self):
        for p in self.pending:
            if not p[2]:
                got = self._await("ok", self.timeout)
                if got[:1] != [str(p[0])]:
                    self._fail(f"answered slot {got[:1]} where slot {p[0]} was expected")
                p[2] = True
                return

    def collect(self, device):
        """Features of the oldest request as fp32 (B, 1, L, d_model) on `device`."""
        if self.failed:
            raise CaptionWorkerError(self.failed)
        if not self.pending:
            raise RuntimeError("caption worker: nothing was submitted")
        if not self.pending[0][2]:
            self._finish_oldest()
        slot, B, _ = self.pending.pop(0)
        feats = self._view(2 + slot, torch.bfloat16, B * self.L * self.d_model)
        y = feats.to(device).float().view(B, 1, self.L, self.d_model)     # a pageable-memory copy: complete on return, the slot is free again
        del feats
        return y


class CaptionEncoder:
    """CaptionEncoder(t5_path, tokenizer=None, model_max_length=300, device='cuda').encode(texts) -> (y, mask); see the module docstring.

    t5_path: a transformers T5 directory (config.json + weights; T5Encoder.from_pretrained).  tokenizer: any callable with the transformers tokenizer call
    signature returning 'input_ids' and 'attention_mask'; None loads AutoTokenizer from t5_path.  max_batch sizes the worker's shared block
    (2 * max_batch * L * d_model * 2 bytes of features: 79 MB at 16 captions of 300 tokens).  timeout / start_timeout: the worker's time limits in seconds.
    worker: None takes the worker exactly when the process runs the f16 build; True takes it under the bf16 build as well.
    weight_dtype: None (as stored) or "fp8_e4m3" (T5Encoder.from_pretrained); handed to the worker on its command line."""

    def __init__(self, t5_path, tokenizer=None, model_max_length=300, device="cuda", max_batch=16, timeout=120.0, start_timeout=900.0, worker=None,
                 weight_dtype=None):
        from .encoder import check_weight_dtype
        self.weight_dtype = check_weight_dtype(weight_dtype)
        if tokenizer is None:
            from transformers import AutoTokenizer
            tokenizer = AutoTokenizer.from_pretrained(t5_path)
        self.tokenizer, self.model_max_length = tokenizer, int(model_max_length)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.in_process = lib.OPERAND == "bf16" if worker is None else not worker      # worker=True: the worker under the bf16 build too (tests, benchmarks)
        if self.in_process and lib.OPERAND != "bf16":
            raise ValueError("CaptionEncoder(worker=False) under the f16 build: the T5 encoder needs bf16 operands, which this process does not have")
        self.encoder = self.worker = None
        self._tickets = []
        if self.in_process:
            from .encoder import T5Encoder
            self.encoder = T5Encoder.from_pretrained(t5_path, device=self.device, weight_dtype=weight_dtype)
        else:
            self.worker = _Worker(t5_path, self.model_max_length, self.device.index or 0, int(max_batch), float(timeout), float(start_timeout),
                                  weight_dtype=weight_dtype)

    def submit(self, texts):
        """Tokenise and start encoding; returns the host mask.  At most two submits may be outstanding; collect() returns them in order."""
        ids, mask = tokenize(self.tokenizer, texts, self.model_max_length)
        if self.in_process:
            self._tickets.append(self.encoder(ids, mask)[:, None])
        else:
            self.worker.submit(ids, mask)
            self._tickets.append(None)
        return mask

    @property
    def outstanding(self):
        """Submits not collected yet."""
        return len(self._tickets)

    def collect(self):
        y = self._tickets.pop(0)
        return y if self.in_process else self.worker.collect(self.device)

    def encode(self, texts):
        mask = self.submit(texts)
        return self.collect(), mask

    def close(self):
        if self.worker is not None:
            self.worker.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ------------------------------------------------------------------------------------------------ the worker's program
def _worker_main(argv):
    import argparse
    import signal
    from multiprocessing import resource_tracker, shared_memory
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--t5-path", required=True)
    ap.add_argument("--shm", required=True)
    ap.add_argument("--length", type=int, required=True)
    ap.add_argument("--max-batch", type=int, required=True)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--weight-dtype", default=None)
    a = ap.parse_args(argv)
    assert lib.OPERAND == "bf16", "the caption worker must run under the bf16-operand build"
    signal.signal(signal.SIGTERM, lambda *_: sys.exit(143))          # leave through the interpreter's own shutdown, not in the middle of a call
    out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)                                                     # whatever a library prints goes to stderr; the protocol keeps its own stream
    from .encoder import T5Encoder
    torch.cuda.set_device(a.device)
    dev = torch.device("cuda", a.device)
    enc = T5Encoder.from_pretrained(a.t5_path, device=dev, weight_dtype=a.weight_dtype)
    L, D = a.length, enc.config.d_model
    offsets, size = _shm_layout(a.max_batch, L, D)
    shm = shared_memory.SharedMemory(name=a.shm)
    try:                                                              # the parent owns the block: attaching must not make this process unlink it at exit
        resource_tracker.unregister(shm._name, "shared_memory")
    except Exception:      # noqa: BLE001
        pass
    assert shm.size >= size, (shm.size, size)
    print(f"{TAG} ready {D}", file=out, flush=True)
    try:
        for line in sys.stdin:
            parts = line.split()
            if parts[:1] != [TAG]:
                continue
            slot, B = int(parts[1]), int(parts[2])
            assert slot in (0, 1) and 1 <= B <= a.max_batch
            ids = torch.frombuffer(shm.buf, dtype=torch.int32, count=B * L, offset=offsets[0]).view(B, L).clone()
            mask = torch.frombuffer(shm.buf, dtype=torch.int32, count=B * L, offset=offsets[1]).view(B, L).clone()
            y = enc(ids.long(), mask.long()).to(torch.bfloat16).reshape(-1)
            dst = torch.frombuffer(shm.buf, dtype=torch.bfloat16, count=B * L * D, offset=offsets[2 + slot])
            dst.copy_(y)                                              # device -> host, complete on return
            del dst, ids, mask
            print(f"{TAG} ok {slot}", file=out, flush=True)
    finally:
        shm.close()


if __name__ == "__main__":
    _worker_main(sys.argv[1:])
