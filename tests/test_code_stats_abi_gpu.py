"""The four writing entry points of include/vtc_stats.h, three ways (modelled
on tests/test_ssim_abi_gpu.py, with the same runners):

  fenced   tests/test_image_abi_fences_gpu.run_case as it is: a plain call,
           then inputs, outputs and workspace inside [guard | payload | guard]
           arenas (tests/fences.py), outputs and workspace 0xFF-filled, the
           workspace of EXACTLY the queried size, every output element written
           (so the call itself zeroes `counts`); one byte less workspace must
           answer VTC_ERR_WORKSPACE and touch nothing
  skewed   float32 codes and images 4, 8 and 12 bytes past a 16-byte boundary,
           float64 images 8; the int64 and float64 arrays 8, the other 4-byte
           arrays 4
  held     on a side stream behind a delay (tests/held_stream.py), every
           payload poisoned until the stream uploads the inputs, canaries on
           the null stream before and after the call; bitwise the
           default-stream result

The cases: 257 x 70 codes (rows past one block of 256 threads' rows, columns
past one 64-wide tile) with 7 and 1000 bins, three pairs at 16 bins, and
3 x 17 x 33 images with 6 bins.  No column, pair or bin is empty: an empty one
answers NaN, which the runners' torch.equal cannot compare
(tests/test_code_stats_gpu.py covers those).  The truth is numpy, computed
here.
"""
import ctypes

import numpy as np
import pytest
import torch

import fences
import held_stream
import test_image_abi_fences_gpu as image_table
import test_jpeg_abi_gpu as codec_table

pytestmark = pytest.mark.gpu

OK = 0
F32, F64 = 0, 2
B, S = 257, 70
BOUND = 1e-11   # float64 sums of <= 257 terms: 257 * 2^-53 = 2.9e-14
Case, Spec = image_table.Case, image_table.Spec

CASES = []


def case(entry, name):
  def deco(make):
    CASES.append(Case(entry, name, make))
    return make
  return deco


def padded(nbytes):
  return -(-nbytes // 256) * 256


def _codes():
  rs = np.random.RandomState(257)
  x = rs.laplace(size=(B, S)).astype(np.float32)
  x[rs.rand(B, S) < 0.5] = 0.0
  x[:, 7] = (rs.randint(-20, 21, size=B) * 0.25).astype(np.float32)
  assert ((x != 0).sum(0) > 1).all()
  return x


IGNORE = np.zeros(1, np.float32)


def _kept(x, c):
  return x[:, c][x[:, c] != 0].astype(np.float64)


@case('vtc_code_summary', '257x70')
def _summary_case(lib):
  x = _codes()
  ws = lib.vtc_code_summary_workspace_bytes(B, S)
  assert ws == padded(8 * S) + 4 * padded(4 * S)

  def call(lib, p, ws_ptr, ws_bytes, stream):
    return lib.vtc_code_summary(p['codes'], B, S, p['ignore'], 1, p['kept'],
                                p['lo'], p['hi'], p['mean'], p['var'],
                                p['nonfinite'], ws_ptr, ws_bytes, stream)

  def truth(res, inputs):
    for c in range(S):
      k = _kept(inputs['codes'], c)
      assert res['kept'][c] == len(k) and res['nonfinite'][c] == 0
      assert res['lo'][c] == k.min() and res['hi'][c] == k.max()
      assert abs(res['mean'][c] - k.mean()) <= BOUND * np.abs(k).mean()
      assert abs(res['var'][c] - k.var()) <= BOUND * k.var()

  outputs = {'kept': ((S,), np.int64), 'nonfinite': ((S,), np.int64)}
  outputs.update({k: ((S,), np.float64) for k in ('lo', 'hi', 'mean', 'var')})
  return Spec({'codes': x, 'ignore': IGNORE}, outputs, call, truth, ws)


def _histogram_case(bins):
  def make(lib):
    x = _codes()
    lo = np.array([_kept(x, c).min() for c in range(S)])
    hi = np.array([_kept(x, c).max() for c in range(S)])
    ws = lib.vtc_code_histogram_workspace_bytes(B, S, bins)
    assert ws == 2 * padded(8 * S)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_code_histogram(p['codes'], B, S, p['ignore'], 1, p['lo'],
                                    p['hi'], bins, p['counts'], ws_ptr,
                                    ws_bytes, stream)

    def truth(res, inputs):
      for c in range(S):
        want = np.histogram(_kept(inputs['codes'], c),
                            np.linspace(lo[c], hi[c], bins + 1))[0]
        assert np.array_equal(res['counts'][c], want), c

    return Spec({'codes': x, 'ignore': IGNORE, 'lo': lo, 'hi': hi},
                {'counts': ((S, bins), np.int64)}, call, truth, ws)
  return make


case('vtc_code_histogram', '257x70-7bins')(_histogram_case(7))
case('vtc_code_histogram', '257x70-1000bins')(_histogram_case(1000))


@case('vtc_code_joint_histogram', '257x70-3pairs-16bins')
def _joint_case(lib):
  x = _codes()
  pairs = np.array([(0, 1), (69, 7), (5, 5)], np.int32)
  bins = 16
  ws = lib.vtc_code_joint_histogram_workspace_bytes(B, len(pairs))
  assert ws == 5 * padded(4 * len(pairs))

  def call(lib, p, ws_ptr, ws_bytes, stream):
    return lib.vtc_code_joint_histogram(
        p['codes'], B, S, p['pairs'], len(pairs), S, p['ignore'], 1, bins,
        p['kept'], p['lo'], p['hi'], p['counts'], ws_ptr, ws_bytes, stream)

  def truth(res, inputs):
    codes = inputs['codes']
    for n, (i, j) in enumerate(pairs):
      keep = (codes[:, i] != 0) & (codes[:, j] != 0)
      a, b = codes[keep, i].astype(np.float64), codes[keep, j].astype(
          np.float64)
      assert len(a) > 1 and res['kept'][n] == len(a)
      assert res['lo'][n].tolist() == [a.min(), b.min()]
      assert res['hi'][n].tolist() == [a.max(), b.max()]
      want = np.histogram2d(a, b, bins=[
          np.linspace(a.min(), a.max(), bins + 1),
          np.linspace(b.min(), b.max(), bins + 1)])[0]
      assert np.array_equal(res['counts'][n], want), (i, j)

  return Spec({'codes': x, 'pairs': pairs, 'ignore': IGNORE},
              {'kept': ((len(pairs),), np.int64),
               'lo': ((len(pairs), 2), np.float64),
               'hi': ((len(pairs), 2), np.float64),
               'counts': ((len(pairs), bins, bins), np.int64)}, call, truth,
              ws)


def _binned_case(dtype):
  def make(lib):
    count, h, w, nbins = 3, 17, 33, 6
    rs = np.random.RandomState(17 + dtype)
    images = rs.randn(count, h, w).astype(
        np.float32 if dtype == F32 else np.float64)
    bin_of = rs.randint(-1, nbins + 1, size=(h, w)).astype(np.int32)
    assert all((bin_of == k).any() for k in range(-1, nbins + 1))
    ws = lib.vtc_binned_mean_workspace_bytes(count, h, w, nbins)
    assert ws == padded(8 * count * nbins) + padded(4 * nbins)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_binned_mean(p['images'], dtype, p['bin_of'], count, h, w,
                                 nbins, p['means'], p['members'], ws_ptr,
                                 ws_bytes, stream)

    def truth(res, inputs):
      x = inputs['images'].astype(np.float64)
      for k in range(nbins):
        assert res['members'][k] == (bin_of == k).sum()
        for i in range(count):
          picked = x[i][bin_of == k]
          assert abs(res['means'][i, k] - picked.mean()) <= (
              BOUND * np.abs(picked).mean())

    return Spec({'images': images, 'bin_of': bin_of},
                {'means': ((count, nbins), np.float64),
                 'members': ((nbins,), np.int64)}, call, truth, ws)
  return make


case('vtc_binned_mean', '3x17x33-f32-6bins')(_binned_case(F32))
case('vtc_binned_mean', '3x17x33-f64-6bins')(_binned_case(F64))

IDS = [c.id for c in CASES]


def test_every_writing_entry_point_has_a_row():
  import vtc_hip
  writing = {name for name in vtc_hip.STATS_SIGNATURES
             if not name.endswith(('_workspace_bytes', '_abi_version'))}
  assert writing == {c.entry for c in CASES} and len(writing) == 4


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_fenced(device, c):
  image_table.run_case(device, c)


# --------------------------------------------------------- skewed pointers
# float64 needs 8-byte alignment: 8 is its only skew
SKEWED = [(c, skew) for c in CASES
          for skew in ((8,) if '-f64-' in c.id else (4, 8, 12))]


@pytest.mark.parametrize('c,main_skew', SKEWED,
                         ids=['%s+%d' % (c.id, skew) for c, skew in SKEWED])
def test_skewed(device, c, main_skew):
  import vtc_hip
  lib = vtc_hip.load_library()
  spec = c.make(lib)
  stream = vtc_hip.current_stream(device)
  want, _ = codec_table._plain(device, lib, spec, stream)
  spec.truth({k: v.cpu().numpy() for k, v in want.items()}, spec.inputs)

  t, f = {}, {}
  for k, v in spec.inputs.items():
    skew = main_skew if k in ('codes', 'images') else v.dtype.itemsize
    t[k], f[k] = fences.fenced_copy(v, device, skew=skew)
    assert t[k].data_ptr() % 16 == skew
  for k, (shape, dtype) in spec.outputs.items():   # int64 and float64
    t[k], f[k] = fences.fenced(shape, codec_table._torch_dtype(dtype), device,
                               skew=8)
    assert t[k].data_ptr() % 16 == 8
  ws, f['workspace'] = fences.fenced_workspace(spec.ws_bytes, device)
  pointers = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}
  rc = spec.call(lib, pointers, ctypes.c_void_p(ws.data_ptr()), spec.ws_bytes,
                 stream)
  torch.cuda.synchronize(device)
  assert rc == OK, '%s skewed: %s' % (c.id, lib.vtc_last_error())
  for k, fence in f.items():
    fence.assert_intact('%s (+%d): %s' % (c.id, main_skew, k))
  for k, v in spec.inputs.items():
    assert np.array_equal(t[k].cpu().numpy(), v), k
  for k, v in want.items():
    if t[k].dtype.is_floating_point:
      f[k].assert_written('%s (+%d): %s' % (c.id, main_skew, k))
    assert torch.equal(t[k], v), (
        '%s (+%d): %s differs from the plain call in %d elements'
        % (c.id, main_skew, k, int((t[k] != v).sum())))


# ------------------------------------------------------------ held stream
@pytest.fixture(scope='module')
def hold(device):
  """The shared delay, raised (never lowered) to ten times the slowest
  host-side enqueue of this table, each call timed on its second run."""
  import vtc_hip
  lib = vtc_hip.load_library()
  h = held_stream.hold(device)
  stream = vtc_hip.current_stream(device)
  largest = h.largest_enqueue_ms or 0.0
  for c in CASES:
    spec = c.make(lib)
    codec_table._plain(device, lib, spec, stream)
    largest = max(largest, codec_table._plain(device, lib, spec, stream)[1])
  h.set_delay(largest)
  print('code_stats_abi_delay %s' % h.describe())
  return h


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_held_side_stream(device, hold, c):
  codec_table.test_held_side_stream(device, hold, c)
