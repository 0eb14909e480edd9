"""The fifth header, include/vtc_quality.h, held to what tests/
test_jpeg_decode_host.py asks of the fourth: QUALITY_SIGNATURES is exactly the
declared surface and shares no name with the other four tables, the library
exports it, the five version numbers, the workspace query term for term, bad
arguments answered before any device work; the numpy restatement
tests/ssim_oracle.py against tests/golden/ssim.npz (scipy's filter); the error
mapping of utils.plotting.  No GPU needed."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import helpers
import ssim_oracle

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'vtc_quality.h'
OTHER_HEADERS = [REPO / 'include' / name
                 for name in ('vtc_hip.h', 'vtc_image.h', 'vtc_codec.h',
                              'vtc_decode.h')]

OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, 1, 2, 3
F32, F64 = 0, 2
# what tools/make_ssim_golden.py found between scipy's filter and the numpy
# tap sum was 1.7e-13 at most
HELPER_BOUND = 1e-11


def _code(path):
  return re.sub(r'/\*.*?\*/', '', path.read_text(), flags=re.S)


def declarations():
  """name -> argument text of every function include/vtc_quality.h declares."""
  return {m.group(1): m.group(2)
          for m in re.finditer(r'\b(vtc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;',
                               _code(HEADER))}


def _lib():
  import vtc_hip
  return vtc_hip, vtc_hip.load_library()


def test_header_is_parsed():
  assert sorted(declarations()) == [
      'vtc_quality_abi_version', 'vtc_ssim', 'vtc_ssim_workspace_bytes']
  assert re.search(r'#define\s+VTC_QUALITY_ABI_VERSION\s+1\b', _code(HEADER))
  assert re.search(r'\bVTC_DTYPE_F64\s*=\s*2\b', _code(HEADER))


def test_the_five_headers_do_not_overlap():
  for other in OTHER_HEADERS:
    names = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(other)))
    assert names and not names & set(declarations()), other.name


def test_binding_table_is_the_declared_surface():
  vtc_hip, lib = _lib()
  assert sorted(vtc_hip.QUALITY_SIGNATURES) == sorted(declarations())
  for other in (vtc_hip.SIGNATURES, vtc_hip.IMAGE_SIGNATURES,
                vtc_hip.CODEC_SIGNATURES, vtc_hip.DECODE_SIGNATURES):
    assert not set(vtc_hip.QUALITY_SIGNATURES) & set(other)
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declarations().items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.QUALITY_SIGNATURES[name][1]) == count, name
    assert getattr(lib, name).argtypes == vtc_hip.QUALITY_SIGNATURES[name][1]
  assert lib.vtc_quality_abi_version() == vtc_hip.QUALITY_ABI_VERSION == 1
  assert vtc_hip.DTYPE_F64 == F64 and vtc_hip.DTYPE_F32 == F32
  # the other four versions stay where they were
  assert lib.vtc_abi_version() == 4
  assert lib.vtc_image_abi_version() == 1
  assert lib.vtc_codec_abi_version() == 1
  assert lib.vtc_decode_abi_version() == 1


def test_workspace_query_is_stated_term_for_term():
  """One float64 per 16 x 32 output tile of every image, rounded up to 256
  bytes; host-only; 0 for a shape the call refuses."""
  _, lib = _lib()
  query = lib.vtc_ssim_workspace_bytes

  def padded(nbytes):
    return -(-nbytes // 256) * 256

  for count, h, w in ((1, 11, 11), (1, 16, 32), (1, 17, 33), (3, 12, 17),
                      (2, 640, 1280), (2, 641, 1281), (64, 256, 256)):
    tiles = -(-h // 16) * -(-w // 32)
    assert query(count, h, w) == padded(8 * count * tiles), (count, h, w)
  assert query(2, 640, 1280) == 2 * 40 * 40 * 8
  assert query(2, 641, 1281) == padded(2 * 41 * 41 * 8)
  for count, h, w in ((0, 16, 32), (-1, 16, 32), (1, 10, 32), (1, 32, 10),
                      (1, 0, 0)):
    assert query(count, h, w) == 0


def _refused(lib, rc, status, *words):
  assert rc == status, (rc, lib.vtc_last_error())
  text = lib.vtc_last_error().decode()
  for word in words:
    assert word in text, text


def test_argument_errors_do_not_touch_the_gpu():
  """Null pointers, count = 0, an unknown dtype, h = 10 or w = 10, a short or
  missing workspace and an aliased map come back before any HIP call: this
  runs with no device.  The non-null pointers are host integers that are never
  dereferenced."""
  _, lib = _lib()
  x, y, rng, mean, smap, ws = (ctypes.c_void_p(v << 20) for v in range(1, 7))
  need = lib.vtc_ssim_workspace_bytes(3, 12, 17)
  assert need == 256
  ssim = lib.vtc_ssim
  #       x  y  dtype range mean map  count h  w   ws  bytes stream
  good = [x, y, F32, rng, mean, smap, 3, 12, 17, ws, need, None]
  for position in (0, 1, 3, 4):
    args = list(good)
    args[position] = None
    _refused(lib, ssim(*args), ERR_INVALID_ARGUMENT, 'vtc_ssim', 'null')
  for position, value, word in ((6, 0, 'count = 0'), (6, -2, 'count = -2'),
                                (2, 1, 'dtype 1'), (2, 3, 'dtype 3'),
                                (7, 0, 'h = 0')):
    args = list(good)
    args[position] = value
    _refused(lib, ssim(*args), ERR_INVALID_ARGUMENT, 'vtc_ssim', word)
  for position, word in ((7, 'h = 10'), (8, 'w = 10')):
    args = list(good)
    args[position] = 10
    _refused(lib, ssim(*args), ERR_UNSUPPORTED, 'vtc_ssim', word)
  args = list(good)
  args[10] = need - 1
  _refused(lib, ssim(*args), ERR_WORKSPACE, 'workspace',
           '%d bytes, %d needed' % (need - 1, need))
  args = list(good)
  args[9] = None
  _refused(lib, ssim(*args), ERR_WORKSPACE, 'workspace')
  # the map over an input, or starting inside one
  for dtype, clash in ((F32, x), (F64, y),
                       (F64, ctypes.c_void_p((2 << 20) + 3 * 12 * 17 * 8 - 8))):
    args = list(good)
    args[2], args[5] = dtype, clash
    _refused(lib, ssim(*args), ERR_INVALID_ARGUMENT, 'vtc_ssim', 'alias')
  # right behind a float32 input is no overlap: it gets as far as the
  # workspace check
  args = list(good)
  args[5], args[10] = ctypes.c_void_p((1 << 20) + 3 * 12 * 17 * 4), 0
  _refused(lib, ssim(*args), ERR_WORKSPACE, 'workspace')


def test_numpy_restatement_reproduces_the_fixture():
  """Every map and mean of tests/golden/ssim.npz, which scipy's
  gaussian_filter wrote, from the tap sum with the fold rule."""
  g = helpers.load('ssim')
  cases = [str(c) for c in g['cases']]
  assert len(cases) == 28 and len(set(cases)) == 28
  assert str(g['scipy_version'])
  worst = 0.0
  for tag in cases:
    x, y = g[tag + '_x'], g[tag + '_y']
    assert x.dtype == np.float32 and y.dtype == np.float32
    r, r_none = float(g[tag + '_range']), float(g[tag + '_range_none'])
    assert r_none == float(x.max() - x.min()) == ssim_oracle.derived_range(x)
    for bound in (r, r_none):   # the condition the 1e-9 device bound rests on
      assert max(np.abs(x).max(), np.abs(y).max()) <= 2 * bound, tag
    mean, smap = ssim_oracle.ssim(x, y, r)
    assert smap.shape == x.shape and smap.dtype == np.float64
    gap = max(abs(mean - float(g[tag + '_mean'])),
              float(np.abs(smap - g[tag + '_map']).max()))
    mean_none, _ = ssim_oracle.ssim(x, y)
    gap = max(gap, abs(mean_none - float(g[tag + '_mean_none'])))
    worst = max(worst, gap)
    assert gap < HELPER_BOUND, (tag, gap)
  print('ssim_oracle_vs_scipy worst %.2e' % worst)


def test_restatement_edges():
  rs = np.random.RandomState(3)
  x = rs.rand(13, 19)
  mean, smap = ssim_oracle.ssim(x, x, 1.0)
  assert mean == 1.0 and (smap == 1.0).all()
  with pytest.raises(ValueError):
    ssim_oracle.ssim(rs.rand(10, 40), rs.rand(10, 40), 1.0)
  # a window that reflects on both sides at once
  assert ssim_oracle.fold(np.arange(-5, 8), 3).tolist() == [
      1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]
  assert abs(ssim_oracle.gaussian_taps().sum() - 1.0) < 1e-15
  assert len(ssim_oracle.gaussian_taps()) == 11


def test_error_mapping_of_the_python_layer():
  import torch
  import vtc_hip
  from utils import jpeg
  from utils import plotting
  a, b = torch.zeros(12, 17), torch.zeros(12, 17)
  with pytest.raises(vtc_hip.VtcHipError):
    plotting.compute_ssim(a, b)
  with pytest.raises(vtc_hip.VtcHipError):
    plotting.compute_ssim(a.double(), b.double(), 1.0)
  with pytest.raises(vtc_hip.VtcHipError):
    plotting.compute_ssim_images(a[None], b[None], [1.0], return_map=True)
  # the reference's ValueError below 11 per side, before anything else
  with pytest.raises(ValueError):
    plotting.compute_ssim(torch.zeros(10, 40), torch.zeros(10, 40))
  with pytest.raises(ValueError):
    plotting.compute_ssim(torch.zeros(40, 10), torch.zeros(40, 10), 1.0)
  with pytest.raises(ValueError):
    plotting.compute_ssim_images(torch.zeros(2, 10, 40),
                                 torch.zeros(2, 10, 40))
  with pytest.raises(ValueError):
    plotting.compute_ssim(torch.zeros(3, 12, 17), torch.zeros(3, 12, 17))
  with pytest.raises(TypeError):
    plotting.compute_ssim(np.zeros((12, 17)), np.zeros((12, 17)))
  with pytest.raises(vtc_hip.VtcHipError):
    jpeg.rate_distortion_image(torch.zeros(16, 16), torch.eye(64), (8, 8),
                               [1.] * 64, 1.0)
