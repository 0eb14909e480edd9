"""Side streams held behind a delay, for the stream-order tests.

A call that is handed stream `s` must put every device operation on `s`.  On
the default (null) stream that cannot be seen: everything lands on one queue.
Here the caller's work sits on a PyTorch pool stream -- created non-blocking, so
it does not synchronise with the null stream -- behind `torch.cuda._sleep`:
whatever the callee puts on another stream runs while `s` still sleeps, before
the caller's staging, and reads or writes poison.

`hold(device)` calibrates the sleep once per process (an event pair around a
fixed cycle count) and hands out at most two side streams, shared by every test
module.  `set_delay` fixes the delay from the largest host-side enqueue time
the caller measured: ten times that, and never less than 20 ms.  The factor is
head-room for host jitter; what proves that a delay was long enough is the
canary each test takes on the null stream (`canary` / `is_poison`).
"""
import time

import torch

import fences

CALIBRATION_CYCLES = 1000000
MIN_DELAY_MS = 20.0
HEAD_ROOM = 10.0


class Hold(object):
  def __init__(self, device):
    self.device = device
    self.streams = [torch.cuda.Stream(device), torch.cuda.Stream(device)]
    s = self.streams[0]
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
      torch.cuda._sleep(1000)                   # first use: module load
      start.record()
      torch.cuda._sleep(CALIBRATION_CYCLES)
      end.record()
    end.synchronize()
    self.calibration_ms = start.elapsed_time(end)
    self.cycles_per_ms = CALIBRATION_CYCLES / self.calibration_ms
    self.largest_enqueue_ms = None
    self.set_delay(0.0)

  def set_delay(self, largest_enqueue_ms):
    self.largest_enqueue_ms = largest_enqueue_ms
    self.delay_ms = max(MIN_DELAY_MS, HEAD_ROOM * largest_enqueue_ms)
    self.cycles = int(self.delay_ms * self.cycles_per_ms)

  def sleep(self):
    """Enqueue the delay on the current stream."""
    torch.cuda._sleep(self.cycles)

  def measured_delay_ms(self):
    """The delay as the device sees it (one held stream, nothing behind)."""
    s = self.streams[0]
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
      start.record()
      self.sleep()
      end.record()
    end.synchronize()
    return start.elapsed_time(end)

  def describe(self):
    return ('_sleep(%d) = %.3f ms (%.0f cycles per ms); largest enqueue '
            '%.3f ms; delay %.1f ms = _sleep(%d)'
            % (CALIBRATION_CYCLES, self.calibration_ms, self.cycles_per_ms,
               self.largest_enqueue_ms, self.delay_ms, self.cycles))


_HOLD = {}


def hold(device):
  key = str(device)
  if key not in _HOLD:
    _HOLD[key] = Hold(device)
  return _HOLD[key]


def poisoned_like(value, device):
  """(tensor, pinned): a 0xFF-filled device tensor shaped like `value` and the
  value in pinned host memory, to be uploaded on the held stream."""
  value = value.detach().cpu().contiguous()
  t = torch.empty(value.shape, dtype=value.dtype, device=device)
  _bytes(t).fill_(fences.POISON_BYTE)
  return t, value.pin_memory()


def _bytes(t):
  """A contiguous tensor's storage as a flat uint8 view."""
  if t.is_complex():
    t = torch.view_as_real(t)
  return t.reshape(-1).view(torch.uint8)


def canary_word(t):
  """A 4-byte (or shorter) view of the first bytes of `t`, as uint8."""
  raw = _bytes(t)
  return raw[:min(4, raw.numel())]


def canary(t):
  """Enqueue, on the NULL stream, a copy of the first word of `t`."""
  with torch.cuda.stream(torch.cuda.default_stream(t.device)):
    return canary_word(t).clone()


def is_poison(word):
  return bool((word.cpu() == fences.POISON_BYTE).all())


def timed(fn):
  start = time.perf_counter()
  out = fn()
  return out, (time.perf_counter() - start) * 1e3
