"""Every writing entry point of include/vtc_image.h behind guard bands
(tests/fences.py), with the discipline tests/test_abi_fences_gpu.py and
tests/test_pointer_alignment_gpu.py give the first header.

Each case calls the raw ctypes function four times:

  plain    ordinary tensors, zero-filled outputs, a roomy zeroed workspace
  fenced   inputs, outputs and workspace inside [guard | payload | guard]
           arenas, outputs and workspace 0xFF-filled, the workspace of
           EXACTLY the queried size
  skewed   the same with every data pointer moved to its element alignment
           only (4 / 8 / 12 bytes past a 16-byte boundary for float32 and
           int32, 8 for float64, 3 for uint8); the workspace keeps its
           256-byte alignment, as the header asks
  short    one byte less workspace than queried (where there is one): the
           call must answer VTC_ERR_WORKSPACE and touch nothing

and asserts status, every guard intact, inputs bitwise unchanged, float
outputs fully written, and torch.equal with the plain call.  One truth check
per case against numpy (float64 for the filters, helpers.rel_err < 1e-6;
exact for the moves) keeps two identically wrong calls from passing.

CASES is imported as data by tests/test_image_abi_host.py, which fails when a
writing entry point of the header has no row here.
"""
import ctypes

import numpy as np
import pytest
import torch

import fences
import helpers

pytestmark = pytest.mark.gpu

OK, ERR_WORKSPACE = 0, 3
F32, U8 = 0, 1
H, W, C = 37, 53, 2


class Case(object):
  def __init__(self, entry, name, make):
    self.entry, self.name, self.make = entry, name, make
    self.id = '%s-%s' % (entry[4:], name)


class Spec(object):
  """inputs: name -> numpy array; outputs: name -> (shape, numpy dtype);
  call(lib, pointers, ws_ptr, ws_bytes, stream) -> status; truth(results,
  inputs) -> None (asserts); ws_bytes: the query's answer (0: none)."""

  def __init__(self, inputs, outputs, call, truth, ws_bytes=0):
    self.inputs, self.outputs = inputs, outputs
    self.call, self.truth, self.ws_bytes = call, truth, int(ws_bytes)


CASES = []


def case(entry, name):
  def deco(make):
    CASES.append(Case(entry, name, make))
    return make
  return deco


def _p(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _fold(i, n):
  m = np.mod(i, 2 * n)
  return np.where(m < n, m, 2 * n - 1 - m)


def _image(rs, dtype, count=2):
  if dtype == U8:
    return rs.randint(0, 256, size=(count, H, W, C)).astype(np.uint8)
  return rs.rand(count, H, W, C).astype(np.float32)


def _np_dtype(code):
  return np.uint8 if code == U8 else np.float32


# ------------------------------------------------------------------ cases
def _fd_case(dtype, fh, fw):
  def make(lib):
    rs = np.random.RandomState(fh * 100 + fw + dtype)
    img = _image(rs, dtype)
    filt = rs.randn(fh, fw) + 1j * rs.randn(fh, fw)
    ws = lib.vtc_img_filter_fd_workspace_bytes(2, H, W, C, fh, fw)
    assert ws >= 8 * 2 * C * fh * fw + 16 * 2 * C * fh * (fw // 2 + 1)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_img_filter_fd(p['images'], dtype, p['filter'], p['out'],
                                   2, H, W, C, fh, fw, ws_ptr, ws_bytes,
                                   stream)

    def truth(res, inputs):
      x = inputs['images'].astype(np.float64)
      want = np.real(np.fft.ifft2(
          filt[None, :, :, None] * np.fft.fft2(x, (fh, fw), axes=(1, 2)),
          axes=(1, 2)))[:, :H, :W]
      assert helpers.rel_err(res['out'], want.astype(np.float32)) < 1e-6

    return Spec({'images': img, 'filter': filt.view(np.float64)},
                {'out': ((2, H, W, C), np.float32)}, call, truth, ws)
  return make


case('vtc_img_filter_fd', 'f32-37x53')(_fd_case(F32, 37, 53))
case('vtc_img_filter_fd', 'f32-40x64')(_fd_case(F32, 40, 64))
case('vtc_img_filter_fd', 'u8-41x55')(_fd_case(U8, 41, 55))


def _sd_truth_general(x, filt):
  fh, fw = filt.shape
  x = x.astype(np.float64)
  want = np.zeros(x.shape)
  for j in range(fh):
    rows = _fold(np.arange(H) + (fh - 1) // 2 - j, H)
    for i in range(fw):
      cols = _fold(np.arange(W) + (fw - 1) // 2 - i, W)
      want += filt[j, i] * x[:, rows][:, :, cols]
  return want


def _sd_general_case(dtype, fh, fw):
  def make(lib):
    rs = np.random.RandomState(fh * 100 + fw + dtype)
    img = _image(rs, dtype)
    filt = rs.randn(fh, fw) / (fh * fw)
    assert lib.vtc_img_filter_sd_workspace_bytes(2, H, W, C, fh, fw, 0) == 0

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_img_filter_sd(p['images'], dtype, p['filter'], None,
                                   None, p['out'], 2, H, W, C, fh, fw, ws_ptr,
                                   ws_bytes, stream)

    def truth(res, inputs):
      want = _sd_truth_general(inputs['images'], filt)
      assert helpers.rel_err(res['out'], want.astype(np.float32)) < 1e-6

    return Spec({'images': img, 'filter': filt},
                {'out': ((2, H, W, C), np.float32)}, call, truth, 0)
  return make


case('vtc_img_filter_sd', 'general-f32-5x7')(_sd_general_case(F32, 5, 7))
case('vtc_img_filter_sd', 'general-u8-4x6')(_sd_general_case(U8, 4, 6))
case('vtc_img_filter_sd', 'general-f32-37x53')(_sd_general_case(F32, 37, 53))


def _sd_separable_case(dtype, fh, fw):
  def make(lib):
    rs = np.random.RandomState(fh * 100 + fw + dtype + 7)
    img = _image(rs, dtype)
    vert = rs.rand(fh) / fh     # sums below 1: a uint8 pass stays in range
    horz = rs.rand(fw) / fw
    ws = lib.vtc_img_filter_sd_workspace_bytes(2, H, W, C, fh, fw, 1)
    assert ws == 4 * 2 * H * W * C

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_img_filter_sd(p['images'], dtype, None, p['vert'],
                                   p['horz'], p['out'], 2, H, W, C, fh, fw,
                                   ws_ptr, ws_bytes, stream)

    def truth(res, inputs):
      x = inputs['images'].astype(np.float64)
      mid = np.zeros(x.shape)
      for i in range(fw):
        mid += horz[i] * x[:, :, _fold(np.arange(W) + fw // 2 - i, W)]
      mid = mid.astype(inputs['images'].dtype).astype(np.float64)
      want = np.zeros(x.shape)
      for j in range(fh):
        want += vert[j] * mid[:, _fold(np.arange(H) + fh // 2 - j, H)]
      assert helpers.rel_err(res['out'], want.astype(np.float32)) < 1e-6

    return Spec({'images': img, 'vert': vert, 'horz': horz},
                {'out': ((2, H, W, C), np.float32)}, call, truth, ws)
  return make


case('vtc_img_filter_sd', 'separable-f32-5x3')(_sd_separable_case(F32, 5, 3))
case('vtc_img_filter_sd', 'separable-u8-4x6')(_sd_separable_case(U8, 4, 6))


def _tile_case(dtype):
  def make(lib):
    img = _image(np.random.RandomState(31 + dtype), dtype)
    ny, nx = H // 8, W // 8

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_img_tile_patches(p['images'], dtype, p['patches'], 2, H,
                                      W, C, 8, 8, stream)

    def truth(res, inputs):
      x = inputs['images']
      want = x[:, :ny * 8, :nx * 8].reshape(2, ny, 8, nx, 8, C).transpose(
          0, 1, 3, 2, 4, 5).reshape(2, ny * nx, 8, 8, C)
      assert np.array_equal(res['patches'], want)

    return Spec({'images': img},
                {'patches': ((2, ny * nx, 8, 8, C), _np_dtype(dtype))}, call,
                truth)
  return make


case('vtc_img_tile_patches', 'f32-8x8')(_tile_case(F32))
case('vtc_img_tile_patches', 'u8-8x8')(_tile_case(U8))


def _assemble_case(dtype, disjoint):
  def make(lib):
    rs = np.random.RandomState(41 + dtype + 2 * disjoint)
    if disjoint:
      pos = np.array([(i * 8, j * 8) for i in range(4) for j in range(6)
                      if (i + j) % 3], dtype=np.int32)
      pos = pos[rs.permutation(len(pos))]
    else:
      pos = np.array([(0, 0), (4, 4), (2, 9), (4, 4), (20, 30), (17, 27),
                      (29, 45)], dtype=np.int32)
    k = len(pos)
    out_h, out_w = int(pos[:, 0].max()) + 8, int(pos[:, 1].max()) + 8
    if dtype == U8:
      patches = rs.randint(1, 256, size=(k, 8, 8, C)).astype(np.uint8)
    else:
      patches = (rs.rand(k, 8, 8, C) + 0.5).astype(np.float32)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_img_assemble_patches(
          p['patches'], dtype, p['positions'], p['image'], k, 8, 8, C, out_h,
          out_w, disjoint, stream)

    def truth(res, inputs):
      want = np.zeros((out_h, out_w, C), dtype=patches.dtype)
      for q in range(k):
        want[pos[q, 0]:pos[q, 0] + 8, pos[q, 1]:pos[q, 1] + 8] = patches[q]
      assert (want == 0).any()
      assert np.array_equal(res['image'], want)

    return Spec({'patches': patches, 'positions': pos},
                {'image': ((out_h, out_w, C), _np_dtype(dtype))}, call, truth)
  return make


case('vtc_img_assemble_patches', 'disjoint-f32')(_assemble_case(F32, 1))
case('vtc_img_assemble_patches', 'disjoint-u8')(_assemble_case(U8, 1))
case('vtc_img_assemble_patches', 'ordered-f32')(_assemble_case(F32, 0))
case('vtc_img_assemble_patches', 'ordered-u8')(_assemble_case(U8, 0))


def _downsample_case(dtype, factor):
  def make(lib):
    img = _image(np.random.RandomState(51 + dtype + factor), dtype)
    oh, ow = -(-H // factor), -(-W // factor)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_img_downsample(p['images'], dtype, p['out'], 2, H, W, C,
                                    factor, stream)

    def truth(res, inputs):
      assert np.array_equal(res['out'],
                            inputs['images'][:, ::factor, ::factor])

    return Spec({'images': img}, {'out': ((2, oh, ow, C), _np_dtype(dtype))},
                call, truth)
  return make


case('vtc_img_downsample', 'f32-by3')(_downsample_case(F32, 3))
case('vtc_img_downsample', 'u8-by5')(_downsample_case(U8, 5))


# ----------------------------------------------------------------- runner
def _skew(dtype, index):
  """Element alignment only: float32 / int32 arrays take 4, 8, 12 bytes in
  turn, float64 8, uint8 3."""
  size = torch.empty((), dtype=dtype).element_size()
  return fences.skew_for(size, (4, 8, 12)[index % 3] if size == 4 else
                         (8 if size == 8 else 3))


def run_case(device, c):
  import vtc_hip
  lib = vtc_hip.load_library()
  spec = c.make(lib)
  stream = vtc_hip.current_stream(device)

  def arenas(skewed):
    t, f = {}, {}
    for n, (k, v) in enumerate(spec.inputs.items()):
      value = torch.from_numpy(np.ascontiguousarray(v))
      t[k], f[k] = fences.fenced_copy(
          value, device, skew=_skew(value.dtype, n) if skewed else 0)
    for n, (k, (shape, dtype)) in enumerate(spec.outputs.items()):
      dtype = torch.from_numpy(np.zeros(1, dtype)).dtype
      t[k], f[k] = fences.fenced(
          shape, dtype, device,
          skew=_skew(dtype, n + len(spec.inputs)) if skewed else 0)
      if skewed:
        assert t[k].data_ptr() % 16 != 0
    return t, f

  def unchanged(t, label):
    for k, v in spec.inputs.items():
      assert torch.equal(t[k].cpu(), torch.from_numpy(
          np.ascontiguousarray(v))), '%s (%s): input %s was modified' % (
              c.id, label, k)

  # plain
  t0 = {k: helpers.to_dev(v, device).clone() for k, v in spec.inputs.items()}
  for k, (shape, dtype) in spec.outputs.items():
    t0[k] = torch.zeros(shape, device=device,
                        dtype=torch.from_numpy(np.zeros(1, dtype)).dtype)
  ws0 = torch.zeros(2 * spec.ws_bytes + (1 << 20), dtype=torch.uint8,
                    device=device)
  rc = spec.call(lib, {k: _p(v) for k, v in t0.items()}, _p(ws0), ws0.numel(),
                 stream)
  torch.cuda.synchronize(device)
  assert rc == OK, '%s plain: %s' % (c.id, lib.vtc_last_error())
  want = {k: t0[k] for k in spec.outputs}
  spec.truth({k: v.cpu().numpy() for k, v in want.items()}, spec.inputs)

  for label, skewed in (('fenced', False), ('skewed', True)):
    t, f = arenas(skewed)
    ws_ptr, nbytes = ctypes.c_void_p(0), spec.ws_bytes
    if nbytes:
      ws, f['workspace'] = fences.fenced_workspace(nbytes, device)
      ws_ptr = _p(ws)
    rc = spec.call(lib, {k: _p(v) for k, v in t.items()}, ws_ptr, nbytes,
                   stream)
    torch.cuda.synchronize(device)
    assert rc == OK, '%s %s: %s' % (c.id, label, lib.vtc_last_error())
    for k, fence in f.items():
      fence.assert_intact('%s (%s): %s' % (c.id, label, k))
    unchanged(t, label)
    for k in spec.outputs:
      if t[k].dtype.is_floating_point:
        f[k].assert_written('%s (%s): %s' % (c.id, label, k))
      assert torch.equal(t[k], want[k]), (
          '%s (%s): %s differs from the plain call in %d elements'
          % (c.id, label, k, int((t[k] != want[k]).sum())))

  if spec.ws_bytes:
    t, f = arenas(False)
    ws, f['workspace'] = fences.fenced_workspace(spec.ws_bytes - 1, device)
    rc = spec.call(lib, {k: _p(v) for k, v in t.items()}, _p(ws),
                   spec.ws_bytes - 1, stream)
    torch.cuda.synchronize(device)
    assert rc == ERR_WORKSPACE, '%s: one byte short gave %d' % (c.id, rc)
    unchanged(t, 'one byte short')
    for k, fence in f.items():
      fence.assert_intact('%s (one byte short): %s' % (c.id, k))
      if k in spec.outputs or k == 'workspace':
        fence.assert_untouched('%s (one byte short): %s' % (c.id, k))


@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_fenced(device, c):
  run_case(device, c)
