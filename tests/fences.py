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

`skew` (0 by default: byte for byte the layout above) starts the payload that
many bytes further on -- a multiple of the element size below 16 -- so that it
is NOT 16-byte aligned: the flat buffer grows by `skew` bytes, the leading
guard with it, and both guards still touch the payload's first and last byte.
tests/test_pointer_alignment_gpu.py runs the fence table on such payloads.

`fenced_staged(value, device)` is an arena whose payload is left poisoned, with
the value beside it in pinned host memory: tests/test_stream_order_gpu.py
uploads it on a side stream, behind a delay.

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

  def __init__(self, shape, dtype, device, fill=POISON_BYTE, skew=0):
    shape = tuple(int(v) for v in (shape if hasattr(shape, '__len__')
                                   else (shape,)))
    self.itemsize = torch.empty((), dtype=dtype).element_size()
    self.nbytes = int(np.prod(shape, dtype=np.int64)) * self.itemsize
    self.guard = guard_bytes(self.nbytes)
    assert self.guard % GUARD_QUANTUM == 0
    self.skew = int(skew)
    assert 0 <= self.skew <= 15 and self.skew % self.itemsize == 0, skew
    # the payload starts `lead` bytes into the flat buffer, the trailing guard
    # is `guard` bytes long: [guard + skew | payload | guard]
    self.lead = self.guard + self.skew
    self.flat = torch.full((self.lead + self.nbytes + self.guard,),
                           GUARD_BYTE, dtype=torch.uint8, device=device)
    self.raw = self.flat[self.lead:self.lead + self.nbytes]
    self.raw.fill_(fill)
    self.payload = self.raw.view(dtype).reshape(shape)
    assert self.payload.data_ptr() == self.flat.data_ptr() + self.lead
    assert self.payload.is_contiguous()
    if self.skew and self.nbytes:
      assert self.payload.data_ptr() % 16 == (
          self.flat.data_ptr() + self.skew) % 16

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
    lead = self.flat[:self.lead]
    trail = self.flat[self.lead + self.nbytes:]
    out = []
    if not bool((lead == GUARD_BYTE).all()):
      bad = torch.nonzero(lead != GUARD_BYTE)
      out.append('leading guard, %d bytes damaged, nearest %d before the '
                 'payload' % (bad.numel(), self.lead - int(bad.max())))
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


def fenced(shape, dtype, device, fill=POISON_BYTE, skew=0):
  """(payload, fence): `payload` is the tensor to hand to the library."""
  f = Fence(shape, dtype, device, fill, skew)
  return f.payload, f


def fenced_copy(value, device, skew=0):
  """A fenced arena holding a copy of `value` (tensor or numpy array)."""
  if not torch.is_tensor(value):
    value = torch.from_numpy(np.ascontiguousarray(value))
  f = Fence(value.shape, value.dtype, device, skew=skew)
  f.set(value)
  return f.payload, f


def fenced_staged(value, device):
  """(payload, fence, pinned): a fenced arena shaped like `value` whose payload
  still holds the 0xFF poison, and `value` in pinned host memory, for a caller
  that uploads it later on a stream of its own choice
  (tests/test_stream_order_gpu.py)."""
  if not torch.is_tensor(value):
    value = torch.from_numpy(np.ascontiguousarray(value))
  f = Fence(value.shape, value.dtype, device)
  pinned = value.contiguous()
  if f.flat.is_cuda:
    pinned = pinned.pin_memory()
  return f.payload, f, pinned


def fenced_workspace(nbytes, device, skew=0):
  """Scratch of exactly `nbytes` bytes (not rounded up), 0xFF-filled."""
  return fenced((int(nbytes),), torch.uint8, device, skew=skew)


def skew_for(itemsize, want):
  """The allowed skew (a multiple of the element size, 1..15 bytes) nearest to
  `want` bytes; ties go to the smaller one."""
  allowed = range(itemsize, 16, itemsize)
  return min(allowed, key=lambda v: (abs(v - want), v))


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

  for past, label in ((True, 'one byte past'), (False, 'one byte before')):
    payload, fence = fenced((5, 7), torch.float32, device)
    payload.zero_()
    fence.flat[fence.guard + fence.nbytes if past else fence.guard - 1] = 0
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

  value = np.arange(35, dtype=np.float32).reshape(5, 7)
  payload, fence, pinned = fenced_staged(value, device)
  fence.assert_untouched('staged arena before its upload')
  fence.assert_intact('staged arena')
  payload.copy_(pinned)
  assert np.array_equal(payload.cpu().numpy(), value)

  ws, fence = fenced_workspace(1000, device)
  assert ws.numel() == 1000 and fence.guard % GUARD_QUANTUM == 0
  assert fence.guard >= GUARD_MIN
  assert bool((ws == POISON_BYTE).all())
  big = Fence((3 << 20,), torch.uint8, device)
  assert big.guard >= big.nbytes
  return reports


def self_test_skewed(device='cpu'):
  """The same three faults on payloads that start 4, 8 and 12 bytes (float32),
  8 bytes (float64) and 1, 2, 3 bytes (uint8) past the aligned position.
  Returns {(dtype name, skew): [past, before, unwritten or None]}."""
  out = {}
  for dtype, skews in ((torch.float32, (4, 8, 12)), (torch.float64, (8,)),
                       (torch.int32, (4,)), (torch.uint8, (1, 2, 3))):
    for skew in skews:
      plain = Fence((5, 7), dtype, device)
      payload, fence = fenced((5, 7), dtype, device, skew=skew)
      assert payload.is_contiguous() and payload.shape == (5, 7)
      assert payload.data_ptr() - fence.flat.data_ptr() == plain.guard + skew
      assert fence.flat.numel() == plain.flat.numel() + skew
      assert bool((fence.raw == POISON_BYTE).all())
      # both guards touch the payload
      assert int(fence.flat[fence.lead - 1]) == GUARD_BYTE
      assert int(fence.flat[fence.lead + fence.nbytes]) == GUARD_BYTE
      fence.assert_untouched('fresh skewed arena')
      payload.zero_()
      fence.assert_intact('clean skewed arena')
      if dtype.is_floating_point:
        fence.assert_written('clean skewed arena')
      reports = []
      for offset in (fence.lead + fence.nbytes, fence.lead - 1):
        payload, fence = fenced((5, 7), dtype, device, skew=skew)
        payload.zero_()
        fence.flat[offset] = 0
        try:
          fence.assert_intact('skewed')
        except FenceError as e:
          reports.append(str(e))
        else:
          raise AssertionError('skewed fence missed a write at %d' % offset)
      unwritten = None
      if dtype.is_floating_point:
        payload, fence = fenced((5, 7), dtype, device, skew=skew)
        payload.zero_()
        fence.raw[17 * fence.itemsize:18 * fence.itemsize] = POISON_BYTE
        fence.assert_intact('skewed, unwritten element')
        try:
          fence.assert_written('skewed, unwritten element')
        except FenceError as e:
          unwritten = str(e)
        else:
          raise AssertionError('skewed fence missed an unwritten element')
      reports.append(unwritten)
      out[(str(dtype).split('.')[-1], skew)] = reports
  value = np.arange(35, dtype=np.float32).reshape(5, 7)
  payload, fence = fenced_copy(value, device, skew=12)
  assert np.array_equal(payload.cpu().numpy(), value)
  fence.assert_intact('skewed copy')
  ws, fence = fenced_workspace(1000, device)
  assert fence.skew == 0 and fence.lead == fence.guard
  assert [skew_for(4, 12), skew_for(8, 12), skew_for(1, 12), skew_for(2, 12),
          skew_for(8, 8), skew_for(4, 8)] == [12, 8, 12, 12, 8, 8]
  return out
