"""Guard-band arenas for the C ABI tests (tests/test_abi_fences_gpu.py).

`fenced(shape, dtype, device, fill)` places a tensor inside one flat uint8
buffer laid out [guard | payload | guard].  The guards hold the byte 0xA5 and
are compared on the device, as uint8, after the stream is synchronised; the
payload is pre-filled with `fill` bytes (0xFF by default: a NaN pattern in
every float format, -1 in the integer ones), so "every element was written"
is `isfinite(payload).all()`.

Each guard is a multiple of 512 bytes long -- the payload keeps the alignment a
fresh torch.empty would have, so every alignment gate of the library picks its
production route -- and at least max(1 MiB, payload bytes): one whole extra
tile or row block past a ragged tail (32 rows x s floats, 128 x 128 floats)
lands inside it.  That is a condition, not a measurement: a write wilder than
the guard is long (a wrong base pointer, an index that overflowed) can still
land beyond it and escape, and a write that happens to store 0xA5 is not seen.

The module runs on the CPU as well (`self_test`), which is how the suite shows
that the fences bite without a GPU and without touching product code.
"""
import numpy as np
import torch

GUARD_BYTE = 0xA5
POISON_BYTE = 0xFF
GUARD_QUANTUM = 512
GUARD_MIN = 1 << 20


class FenceError(AssertionError):
  pass


def guard_bytes(payload_bytes):
  want = max(GUARD_MIN, int(payload_bytes))
  return -(-want // GUARD_QUANTUM) * GUARD_QUANTUM


class Fence(object):
  """One [guard | payload | guard] arena.  `payload` is the tensor view."""

  def __init__(self, shape, dtype, device, fill=POISON_BYTE):
    shape = tuple(int(v) for v in (shape if hasattr(shape, '__len__')
                                   else (shape,)))
    self.itemsize = torch.empty((), dtype=dtype).element_size()
    self.nbytes = int(np.prod(shape, dtype=np.int64)) * self.itemsize
    self.guard = guard_bytes(self.nbytes)
    assert self.guard % GUARD_QUANTUM == 0
    self.flat = torch.full((2 * self.guard + self.nbytes,), GUARD_BYTE,
                           dtype=torch.uint8, device=device)
    self.raw = self.flat[self.guard:self.guard + self.nbytes]
    self.raw.fill_(fill)
    self.payload = self.raw.view(dtype).reshape(shape)
    assert self.payload.data_ptr() == self.flat.data_ptr() + self.guard

  def set(self, value):
    """Copy a same-shaped tensor or array into the payload."""
    if not torch.is_tensor(value):
      value = torch.from_numpy(np.ascontiguousarray(value))
    self.payload.copy_(value.reshape(self.payload.shape))
    return self

  def broken_guards(self):
    """Names of the guards that no longer hold GUARD_BYTE everywhere, with the
    offset of the first damaged byte relative to the payload."""
    if self.flat.is_cuda:
      torch.cuda.synchronize(self.flat.device)
    lead = self.flat[:self.guard]
    trail = self.flat[self.guard + self.nbytes:]
    out = []
    if not bool((lead == GUARD_BYTE).all()):
      bad = torch.nonzero(lead != GUARD_BYTE)
      out.append('leading guard, %d bytes damaged, nearest %d before the '
                 'payload' % (bad.numel(), self.guard - int(bad.max())))
    if not bool((trail == GUARD_BYTE).all()):
      bad = torch.nonzero(trail != GUARD_BYTE)
      out.append('trailing guard, %d bytes damaged, first %d past the end'
                 % (bad.numel(), int(bad.min())))
    return out

  def assert_intact(self, what):
    broken = self.broken_guards()
    if broken:
      raise FenceError('%s: %s' % (what, '; '.join(broken)))

  def assert_written(self, what):
    """Every element of a floating-point payload is finite, i.e. none still
    holds the 0xFF poison."""
    assert self.payload.dtype.is_floating_point, what
    finite = torch.isfinite(self.payload)
    if not bool(finite.all()):
      bad = torch.nonzero(~finite.reshape(-1))
      raise FenceError('%s: %d of %d elements not written (or not finite), '
                       'first at flat index %d'
                       % (what, bad.numel(), finite.numel(), int(bad.min())))

  def assert_untouched(self, what, fill=POISON_BYTE):
    """The payload still holds its fill byte everywhere."""
    if not bool((self.raw == fill).all()):
      raise FenceError('%s: payload was written' % what)


def fenced(shape, dtype, device, fill=POISON_BYTE):
  """(payload, fence): `payload` is the tensor to hand to the library."""
  f = Fence(shape, dtype, device, fill)
  return f.payload, f


def fenced_copy(value, device):
  """A fenced arena holding a copy of `value` (tensor or numpy array)."""
  if not torch.is_tensor(value):
    value = torch.from_numpy(np.ascontiguousarray(value))
  f = Fence(value.shape, value.dtype, device)
  f.set(value)
  return f.payload, f


def fenced_workspace(nbytes, device):
  """Scratch of exactly `nbytes` bytes (not rounded up), 0xFF-filled."""
  return fenced((int(nbytes),), torch.uint8, device)


def self_test(device='cpu'):
  """Three deliberate faults, each of which the fences must report: one byte
  past a payload, one byte before it, one element left unwritten.  Returns the
  list of messages; raises if a fault goes unreported or a clean arena is
  blamed."""
  reports = []
  payload, fence = fenced((5, 7), torch.float32, device)
  payload.zero_()
  fence.assert_intact('clean arena')
  fence.assert_written('clean arena')

  for offset, label in ((fence.guard + fence.nbytes, 'one byte past'),
                        (fence.guard - 1, 'one byte before')):
    payload, fence = fenced((5, 7), torch.float32, device)
    payload.zero_()
    fence.flat[offset] = 0
    try:
      fence.assert_intact(label)
    except FenceError as e:
      reports.append(str(e))
    else:
      raise AssertionError('fence missed a write ' + label + ' the payload')

  payload, fence = fenced((5, 7), torch.float32, device)
  payload.zero_()
  payload.view(-1)[17] = float('nan')   # what an unwritten element still holds
  fence.raw[17 * 4:18 * 4] = POISON_BYTE
  fence.assert_intact('unwritten element')
  try:
    fence.assert_written('unwritten element')
  except FenceError as e:
    reports.append(str(e))
  else:
    raise AssertionError('fence missed an unwritten element')

  ws, fence = fenced_workspace(1000, device)
  assert ws.numel() == 1000 and fence.guard % GUARD_QUANTUM == 0
  assert fence.guard >= GUARD_MIN
  assert bool((ws == POISON_BYTE).all())
  big = Fence((3 << 20,), torch.uint8, device)
  assert big.guard >= big.nbytes
  return reports
