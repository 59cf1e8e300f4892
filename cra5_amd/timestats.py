"""Per-grid-point statistics over many device frames: mean, standard deviation, minimum and maximum over time
(csrc/timestats.hip through ops.time_accumulate / ops.time_finish).

Definitions, for the frames x_0 .. x_(n-1) (fp32, one shape) in the order they are applied, per element:
  s = sum_t (double)x_t and q = sum_t (double)x_t ** 2, accumulated in float64 one frame after another (x_t ** 2 is exact
  in float64: every update rounds once) - the bits of a sequential numpy float64 loop over the frames;
  mean = float32(s / n)          std = float32(sqrt(max(0, (q - s * s / n) / (n - ddof))))     (all in float64)
  min / max = np.minimum / np.maximum over the frames: NaN if any sample is NaN; the sign of a zero is unspecified.
Non-finite samples are not filtered: they reach mean / std under IEEE rules, as np.mean would report them.
The one-pass std loses about n * 2**-53 * mean**2 / var relative accuracy against the two-pass definition: nothing in
float32 while |mean| / std stays below ~1e5.

Ordering.  Consecutive adds update the same memory, so they must run one after another on the device, and float64
addition does not commute bit for bit, so the order must not depend on thread timing.  `add(x, seq=k)` waits (on the
host, on a condition variable) until add k - 1 has been enqueued or skipped, makes the current stream wait on the event
recorded after add k - 1, launches, records its own event and passes the turn: only the launch happens inside a turn.
The result therefore does not depend on which thread or stream calls first.  A caller that cannot deliver seq k must
`skip(k)` or `abort(exc)`, or the later seqs wait for ever.
"""
import threading

import torch

from . import ops

STATS = ("mean", "std", "min", "max")
_NEEDS = {"mean": ("sum",), "std": ("sum", "sumsq"), "min": ("min",), "max": ("max",)}


def check_stats(stats, ddof=0):
    """-> the requested statistics as a tuple in STATS order.  ValueError for an empty selection, an unknown name, or a
    ddof that is not an integer >= 0."""
    if isinstance(stats, (str, bytes)):
        raise ValueError(f"stats must be a sequence of names from {STATS}, got the string {stats!r}")
    names = list(stats)
    if not names:
        raise ValueError(f"stats: the selection is empty - name some of {STATS}")
    unknown = [s for s in names if s not in STATS]
    if unknown:
        raise ValueError(f"stats: unknown statistic(s) {unknown} (known: {STATS})")
    if isinstance(ddof, bool) or not isinstance(ddof, int) or ddof < 0:
        raise ValueError(f"ddof must be an integer >= 0, got {ddof!r}")
    return tuple(s for s in STATS if s in names)


class TimeStats:
    """Device accumulators of the per-element statistics `stats` over fp32 device frames of `shape`.

        ts = TimeStats(shape, stats=("mean", "std", "min", "max"), device=..., ddof=0)
        ts.add(x)             # in call order
        ts.add(x, seq=k)      # k = 0, 1, 2, ...: applied in seq order whatever thread calls first
        ts.skip(k)            # pass turn k without a frame;   ts.abort(exc): wake every waiter, add / result then raise
        ts.result()           # -> {"n": frames added, stat: fp32 device tensor of `shape`}

    Only the accumulators the statistics need are allocated (mean: sum; std: sum and sumsq; min; max), all of them in
    the constructor.  There is no CPU path: add() refuses host tensors."""

    def __init__(self, shape, stats=STATS, device=None, ddof=0):
        self.stats = check_stats(stats, ddof)
        self.ddof = ddof
        self.shape = tuple(int(v) for v in (shape if hasattr(shape, "__iter__") else (shape,)))
        if not self.shape or any(v < 1 for v in self.shape):
            raise ValueError(f"TimeStats: shape must hold positive sizes, got {shape!r}")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        keep = {a for s in self.stats for a in _NEEDS[s]}
        self.acc = {k: torch.empty(self.shape, device=self.device, dtype=dt) for k, dt in ops.TIME_ACCUMULATORS if k in keep}
        self.n = 0                # frames added
        self._next = 0            # the seq whose turn it is
        self._skipped = set()
        self._last = None         # event after the last launch that touched the accumulators
        self._exc = None
        self._cv = threading.Condition()

    def _check(self, x):
        if not isinstance(x, torch.Tensor):
            raise TypeError("TimeStats.add: the frame must be a torch tensor on the GPU")
        if tuple(x.shape) != self.shape:
            raise ValueError(f"TimeStats.add: the frame is {tuple(x.shape)}, the accumulators {self.shape}")
        if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous():
            raise TypeError("TimeStats.add: the frame must be a contiguous fp32 GPU tensor")
        if x.device != self.device:
            raise ValueError(f"TimeStats.add: the frame is on {x.device}, the accumulators on {self.device}")

    def _pass_turn(self):
        self._next += 1
        while self._next in self._skipped:
            self._skipped.discard(self._next)
            self._next += 1
        self._cv.notify_all()

    def add(self, x, seq=None):
        """Fold frame `x` (contiguous fp32 device tensor of `shape`) in, on the current stream.  seq=None: now, in call
        order.  seq=k: as the k-th turn - blocks until turns 0 .. k - 1 have been taken (added or skipped).  The caller
        keeps `x` unchanged until the stream has run the launch.  An add that raises aborts the object."""
        try:
            self._check(x)
            with self._cv:
                if seq is not None:
                    seq = int(seq)
                    if seq < self._next or seq in self._skipped:
                        raise ValueError(f"TimeStats.add: turn {seq} has already been taken (next is {self._next})")
                    while self._next != seq and self._exc is None:
                        self._cv.wait()
                if self._exc is not None:
                    raise self._exc
                stream = torch.cuda.current_stream(self.device)
                if self._last is not None:
                    stream.wait_event(self._last)
                ops.time_accumulate(x, self.acc, first=self.n == 0)
                ev = torch.cuda.Event()
                ev.record(stream)
                self._last = ev
                self.n += 1
                self._pass_turn()
        except BaseException as e:
            if seq is not None:
                self.abort(e)     # the turn can no longer be taken: nobody may wait for it
            raise

    def skip(self, seq):
        """Turn `seq` will not be taken: the seqs after it do not wait for it."""
        with self._cv:
            seq = int(seq)
            if seq < self._next or seq in self._skipped:
                raise ValueError(f"TimeStats.skip: turn {seq} has already been taken (next is {self._next})")
            if seq == self._next:
                self._pass_turn()
            else:
                self._skipped.add(seq)

    def abort(self, exc):
        """Give up: every add() waiting for its turn, every later add() and result() raise `exc` (the first one given)."""
        with self._cv:
            if self._exc is None:
                self._exc = exc if isinstance(exc, BaseException) else RuntimeError(str(exc))
            self._cv.notify_all()

    def result(self):
        """-> {"n": frames added, and per requested statistic a fp32 device tensor of `shape`}, on the current stream
        (which waits for the last add).  mean / std are fresh tensors; min / max ARE the accumulators (no copy): a later
        add() updates them.  ValueError with nothing added, or with n - ddof < 1 when std is requested."""
        with self._cv:
            if self._exc is not None:
                raise self._exc
            if self.n == 0:
                raise ValueError("TimeStats.result: no frame has been added")
            if "std" in self.stats and self.n - self.ddof < 1:
                raise ValueError(f"TimeStats.result: std with ddof = {self.ddof} needs more than {self.ddof} frame(s), "
                                 f"{self.n} added")
            stream = torch.cuda.current_stream(self.device)
            stream.wait_event(self._last)
            res = {"n": self.n}
            want = tuple(s for s in ("mean", "std") if s in self.stats)
            if want:
                res.update(ops.time_finish(self.acc, self.n, self.ddof, want))
                ev = torch.cuda.Event()
                ev.record(stream)
                self._last = ev       # (a later add must not overwrite the sums under the finish kernel)
            for s in ("min", "max"):
                if s in self.stats:
                    res[s] = self.acc[s]
            return {k: res[k] for k in ("n",) + self.stats}
