"""Both fence tables on a side stream that is held behind a delay.

include/vtc_hip.h and include/vtc_image.h promise that every device operation
of a call is issued on the stream the caller hands in; the plugins hand in
torch.cuda.current_stream(), which inside `with torch.cuda.stream(s):` is not
the default stream.  On the default stream a mistake cannot be seen -- a
hipMemsetAsync, a copy or a launch given 0 lands on the same queue and the
result is right by accident -- so every case of tests/test_abi_fences_gpu.py
and tests/test_image_abi_fences_gpu.py runs again as follows.

  plain    as the fence test makes it, on the default stream -> `want`; it also
           pays every first-use cost (vtc_init, function attributes, plans)
  arenas   inputs, outputs and an exactly-sized workspace inside [guard |
           payload | guard] arenas (tests/fences.py), EVERY payload 0xFF (NaN),
           the real inputs in pinned host memory; device synchronised
  held     on a PyTorch pool stream `s` (non-blocking: it does not wait for the
           null stream, nor the null stream for it), in this order:
           the delay, a second 0xFF fill of outputs and workspace, the
           non-blocking upload of every input, the call with stream = s

Whatever the call puts on another stream runs while `s` still sleeps: a stray
memset is overwritten by the second poison fill, a stray kernel reads NaN
inputs or writes what is re-poisoned.  After s.synchronize(): status VTC_OK,
every guard intact, inputs bitwise unchanged (but for spec.inout), every
floating-point output fully written, torch.equal to the plain call, spec.host
equal.  The float64 truth of each case ran in the fence test and is not
repeated.

Canaries.  Each case proves its own premise.  Immediately before the call the
null stream copies one word of a staged input; for a sync-free call it copies
it again as soon as the call has returned.  Both copies must still hold 0xFF:
the null stream ran ahead of `s` for the whole host-side duration of the call.
A canary with real data fails the case -- it proved nothing.

Calls that read back (early stopping, eps >= 0: hipStreamSynchronize inside
the call; vtc_lambda_max_mirrored, whose case waits for the pinned mirror)
block the host until `s` has caught up, so only the first canary applies and
the case covers the call up to its first read-back.  For them the second
canary is taken all the same and must show REAL data: a case listed as
blocking that does not block is a stale entry of BLOCKS, not a weaker test.

The two FFT entry points keep one plan pair per stream (csrc/patches.hip), so
the plain call cannot pay the plan creation of `s`; they make one unheld call
on `s` first.

The delay: tests/held_stream.py.  The module prints its calibration, the
slowest enqueue, the delay and its wall time (stream_order_delay,
stream_order_summary; run with -s).
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import fences
import held_stream
import helpers
import test_abi_fences_gpu as table
import test_image_abi_fences_gpu as image_table

pytestmark = pytest.mark.gpu

OK = 0
ROWS = ([(table, c) for c in table.CASES] +
        [(image_table, c) for c in image_table.CASES])
IDS = [c.id for _, c in ROWS]
assert len(set(IDS)) == len(IDS)

PLANNED = ('vtc_whiten_center_surround', 'vtc_img_filter_fd')

_wall = {'rows': [], 'seconds': 0.0, 'started': None}


def blocks(c):
  """The call reads back inside: it cannot return before `s` has caught up."""
  return 'eps0' in c.name or c.entry == 'vtc_lambda_max_mirrored'


def _torch_dtype(np_dtype):
  return torch.from_numpy(np.zeros(1, np_dtype)).dtype


def _p(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _spec(c):
  import vtc_hip
  lib = vtc_hip.load_library()
  spec = c.make(lib)
  route = getattr(spec, 'route', None)
  if route is not None:
    route(lib)
  return lib, spec


def _outputs(spec):
  return [k for k, v in spec.outputs.items() if v is not None]


def _plain(device, lib, spec, stream):
  """The plain call of the fence tests, timed on the host.  Returns (result
  tensors, spec.host, milliseconds from call to return)."""
  t = {}
  for k, v in spec.inputs.items():
    t[k] = None if v is None else helpers.to_dev(v, device).clone()
  for k, shape_dtype in spec.outputs.items():
    t[k] = None if shape_dtype is None else torch.zeros(
        shape_dtype[0], dtype=_torch_dtype(shape_dtype[1]), device=device)
  ws = torch.zeros(2 * spec.ws_bytes + (1 << 20), dtype=torch.uint8,
                   device=device)
  pointers = {k: _p(v) for k, v in t.items()}
  torch.cuda.synchronize(device)
  rc, ms = held_stream.timed(
      lambda: spec.call(lib, pointers, _p(ws), ws.numel(), stream))
  torch.cuda.synchronize(device)
  assert rc == OK, 'plain: %s' % lib.vtc_last_error()
  names = _outputs(spec) + list(getattr(spec, 'inout', ()))
  return {k: t[k] for k in names}, dict(getattr(spec, 'host', {})), ms


@pytest.fixture(scope='module')
def hold(device):
  """The delay for this module: every sync-free case's plain call is made
  twice on the default stream, the second one timed from call to return."""
  import vtc_hip
  _wall['started'] = time.perf_counter()
  h = held_stream.hold(device)
  stream = vtc_hip.current_stream(device)
  largest, slowest = 0.0, None
  for _, c in ROWS:
    if blocks(c):
      continue
    lib, spec = _spec(c)
    _plain(device, lib, spec, stream)
    _, _, ms = _plain(device, lib, spec, stream)
    if ms > largest:
      largest, slowest = ms, c.id
  h.set_delay(largest)
  print('stream_order_delay %s (slowest enqueue: %s); measured %.1f ms; '
        'calibration pass %.1f s'
        % (h.describe(), slowest, h.measured_delay_ms(),
           time.perf_counter() - _wall['started']))
  return h


def _canary_source(spec, t):
  """The staged input whose first word the canaries copy: real data that is
  not itself the 0xFF pattern."""
  for k, v in spec.inputs.items():
    if v is None or t[k].numel() == 0:
      continue
    word = np.ascontiguousarray(v).reshape(-1).view(np.uint8)[:4]
    if not (word == fences.POISON_BYTE).all():
      return k
  raise AssertionError('no input word to take a canary of')


def run_held(device, c, hold):
  start = time.perf_counter()
  import vtc_hip
  lib, spec = _spec(c)
  what = c.id
  inout = tuple(getattr(spec, 'inout', ()))
  s = hold.streams[0]
  handle = ctypes.c_void_p(s.cuda_stream)
  assert s.cuda_stream != 0

  want, host_want, _ = _plain(device, lib, spec,
                              vtc_hip.current_stream(device))

  # arenas: every payload poisoned, the inputs wait in pinned memory
  t, f, pinned = {}, {}, {}
  for k, v in spec.inputs.items():
    if v is None:
      t[k] = None
    else:
      t[k], f[k], pinned[k] = fences.fenced_staged(v, device)
  for k, shape_dtype in spec.outputs.items():
    if shape_dtype is None:
      t[k] = None
    else:
      t[k], f[k] = fences.fenced(shape_dtype[0], _torch_dtype(shape_dtype[1]),
                                 device)
  ws_ptr = ctypes.c_void_p(0)
  if spec.ws_bytes > 0:
    ws, f['workspace'] = fences.fenced_workspace(spec.ws_bytes, device)
    ws_ptr = _p(ws)
  pointers = {k: _p(v) for k, v in t.items()}
  refill = [f[k] for k in _outputs(spec)] + (
      [f['workspace']] if spec.ws_bytes > 0 else [])
  source = t[_canary_source(spec, t)]

  def stage():
    for fence in refill:
      fence.raw.fill_(fences.POISON_BYTE)
    for k, host in pinned.items():
      t[k].copy_(host.reshape(t[k].shape), non_blocking=True)

  if c.entry in PLANNED:
    # the plan pair of (s, shape) is made by the first call on s: not held
    with torch.cuda.stream(s):
      stage()
    rc = spec.call(lib, pointers, ws_ptr, spec.ws_bytes, handle)
    assert rc == OK, '%s on s, unheld: %s' % (what, lib.vtc_last_error())
    s.synchronize()
    for fence in f.values():
      fence.raw.fill_(fences.POISON_BYTE)
  torch.cuda.synchronize(device)

  with torch.cuda.stream(s):
    hold.sleep()
    stage()
  before = held_stream.canary(source)
  rc, host_ms = held_stream.timed(
      lambda: spec.call(lib, pointers, ws_ptr, spec.ws_bytes, handle))
  after = held_stream.canary(source)
  s.synchronize()
  torch.cuda.synchronize(device)

  assert held_stream.is_poison(before), (
      '%s proved nothing: the null stream saw the staged input before the '
      'call was made (the delay of %.1f ms was too short, or the streams '
      'synchronised)' % (what, hold.delay_ms))
  if blocks(c):
    assert not held_stream.is_poison(after), (
        '%s is listed as reading back inside the call, but returned while its '
        'stream was still held: take it out of blocks()' % what)
    note = 'canaries ok (first only: covered up to the first read-back)'
  else:
    assert held_stream.is_poison(after), (
        '%s proved nothing: the null stream saw the staged input when the '
        'call returned after %.3f ms (the delay of %.1f ms was too short, or '
        'the call synchronised)' % (what, host_ms, hold.delay_ms))
    note = 'canaries ok'

  assert rc == OK, '%s held: status %d (%s)' % (what, rc,
                                                 lib.vtc_last_error())
  for k, fence in f.items():
    fence.assert_intact('%s (held): %s' % (what, k))
  for k, v in spec.inputs.items():
    if v is not None and k not in inout:
      assert torch.equal(t[k].cpu(), pinned[k].reshape(t[k].shape)), (
          '%s (held): input %s was modified' % (what, k))
  for k, v in want.items():
    got = t[k]
    if got.dtype.is_floating_point:
      f[k].assert_written('%s (held): %s' % (what, k))
    if not torch.equal(got, v):
      differ = got != v
      raise AssertionError(
          '%s (held): %s differs from the default-stream call in %d of %d '
          'elements (%d of them not finite, %d zero)'
          % (what, k, int(differ.sum()), differ.numel(),
             int((~torch.isfinite(got.double()))[differ].sum()),
             int((got == 0)[differ].sum())))
  assert dict(getattr(spec, 'host', {})) == host_want, what
  seconds = time.perf_counter() - start
  _wall['rows'].append(what)
  _wall['seconds'] += seconds
  print('stream_order_row %-60s delay_ms %.1f call_ms %.3f %s'
        % (what, hold.delay_ms, host_ms, note))


@pytest.mark.parametrize('c', [c for _, c in ROWS], ids=IDS)
def test_held_side_stream(device, hold, c):
  run_held(device, c, hold)


def _fft_pair(device, hold, entry, run, make_inputs):
  """A on sa, B on sb, both held, enqueued back to back; each must equal its
  serial default-stream result."""
  import vtc_hip
  lib = vtc_hip.load_library()
  sa, sb = hold.streams
  null = vtc_hip.current_stream(device)
  jobs = []
  for seed, s in ((1, sa), (2, sb)):
    inputs = make_inputs(seed)
    dev = {k: helpers.to_dev(v, device) for k, v in inputs.items()}
    want = run(lib, dev, null)
    torch.cuda.synchronize(device)
    # the plan pair of this stream: made now, not behind the delay
    with torch.cuda.stream(s):
      run(lib, dev, ctypes.c_void_p(s.cuda_stream))
    s.synchronize()
    staged = {k: held_stream.poisoned_like(v, device) for k, v in dev.items()}
    jobs.append((s, staged, want))
  torch.cuda.synchronize(device)
  window = time.perf_counter()
  for s, staged, _ in jobs:
    with torch.cuda.stream(s):
      hold.sleep()
      for t, host in staged.values():
        t.copy_(host, non_blocking=True)
  canaries, got = [], []
  for s, staged, _ in jobs:
    first = next(iter(staged.values()))[0]
    canaries.append(held_stream.canary(first))
    with torch.cuda.stream(s):     # torch allocates the result for stream s
      got.append(run(lib, {k: v[0] for k, v in staged.items()},
                     ctypes.c_void_p(s.cuda_stream)))
    canaries.append(held_stream.canary(first))
  window_ms = (time.perf_counter() - window) * 1e3
  sa.synchronize()
  sb.synchronize()
  torch.cuda.synchronize(device)
  for index, word in enumerate(canaries):
    assert held_stream.is_poison(word), (
        '%s on two streams proved nothing: a stream was released before both '
        'calls were enqueued (canary %d of 4; enqueued in %.3f ms on the host, '
        'delay %.1f ms)' % (entry, index, window_ms, hold.delay_ms))
  for name, (_, _, want), out in zip('AB', jobs, got):
    assert bool(torch.isfinite(out).all()), (entry, name)
    assert torch.equal(out, want), (
        '%s: result %s on its own stream differs from the serial call in %d '
        'elements' % (entry, name, int((out != want).sum())))
  assert not torch.equal(got[0], got[1])
  print('stream_order_pair %s 37x53 x 8 planes on two held streams: both '
        'equal their serial results' % entry)


PAIR_H, PAIR_W, PAIR_PLANES = 37, 53, 8


def test_two_streams_do_not_share_fft_plans_whiten(device, hold):
  """vtc_whiten_center_surround, 37 x 53 (no power of two: the likeliest shape
  to need a hipFFT work area), 8 planes, inputs A on one held stream and B on
  another, enqueued back to back and released together.  That the two
  executions overlap is likely, not guaranteed: this test is a detector.  The
  proof is the plan cache keyed by (device, stream, h, w, batch) in
  csrc/patches.hip."""
  def make_inputs(seed):
    rs = np.random.RandomState(seed)
    return {'images': rs.rand(PAIR_PLANES, PAIR_H, PAIR_W, 1).astype(
        np.float32)}

  def run(lib, dev, stream):
    need = lib.vtc_whiten_center_surround_workspace_bytes(
        PAIR_PLANES, PAIR_H, PAIR_W, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    out = torch.full_like(dev['images'], float('nan'))
    rc = lib.vtc_whiten_center_surround(
        _p(dev['images']), _p(out), PAIR_PLANES, PAIR_H, PAIR_W, 1, 1e-3, 0.9,
        1, _p(ws), need, stream)
    assert rc == OK, lib.vtc_last_error()
    out.workspace = ws              # alive until the streams are synchronised
    return out

  _fft_pair(device, hold, 'vtc_whiten_center_surround', run, make_inputs)


def test_two_streams_do_not_share_fft_plans_filter_fd(device, hold):
  """The same for vtc_img_filter_fd with a 37 x 53 filter spectrum (see
  test_two_streams_do_not_share_fft_plans_whiten: overlap is likely, not
  guaranteed; the keyed cache is the proof)."""
  def make_inputs(seed):
    rs = np.random.RandomState(10 + seed)
    filt = rs.randn(PAIR_H, PAIR_W) + 1j * rs.randn(PAIR_H, PAIR_W)
    return {'images': rs.rand(PAIR_PLANES, PAIR_H, PAIR_W, 1).astype(
                np.float32),
            'filter': np.ascontiguousarray(filt).view(np.float64)}

  def run(lib, dev, stream):
    need = lib.vtc_img_filter_fd_workspace_bytes(
        PAIR_PLANES, PAIR_H, PAIR_W, 1, PAIR_H, PAIR_W)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    out = torch.full_like(dev['images'], float('nan'))
    rc = lib.vtc_img_filter_fd(
        _p(dev['images']), image_table.F32, _p(dev['filter']), _p(out),
        PAIR_PLANES, PAIR_H, PAIR_W, 1, PAIR_H, PAIR_W, _p(ws), need, stream)
    assert rc == OK, lib.vtc_last_error()
    out.workspace = ws
    return out

  _fft_pair(device, hold, 'vtc_img_filter_fd', run, make_inputs)


def test_every_row_was_held(device, hold):
  """Runs after the table (same module, file order): prints the module's
  figures; when the whole table ran before it, no row is missing."""
  total = time.perf_counter() - _wall['started']
  print('stream_order_summary rows %d of %d; %s; held cases %.1f s; module '
        '%.1f s' % (len(_wall['rows']), len(ROWS), hold.describe(),
                    _wall['seconds'], total))
  assert len(ROWS) == len(table.CASES) + len(image_table.CASES)
  if len(_wall['rows']) >= len(ROWS):
    assert sorted(_wall['rows']) == sorted(IDS)
