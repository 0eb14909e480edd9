"""The second header, include/vtc_image.h, held to what tests/
test_capi_exports.py and tests/test_abi_fences_host.py ask of the first: the
binding table IMAGE_SIGNATURES is exactly the declared surface, the library
exports it, every writing entry point has a fenced row in tests/
test_image_abi_fences_gpu.py, and bad arguments are answered before any
device work.  No GPU needed."""
import ctypes
import pathlib
import re

import test_image_abi_fences_gpu as table

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'vtc_image.h'
MAIN_HEADER = REPO / 'include' / 'vtc_hip.h'

# entry points that write no device memory of the caller's, with the reason
EXEMPT = {
    'vtc_image_abi_version': 'returns an integer',
}

OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, 1, 2, 3
F32, U8 = 0, 1


def _code(path):
  return re.sub(r'/\*.*?\*/', '', path.read_text(), flags=re.S)


def declarations():
  """name -> argument text of every function include/vtc_image.h declares."""
  return {m.group(1): m.group(2)
          for m in re.finditer(r'\b(vtc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;',
                               _code(HEADER))}


def needs_a_fence(args):
  """Takes a workspace or at least one pointer it may write through."""
  for arg in args.split(','):
    arg = ' '.join(arg.split())
    if '*' not in arg:
      continue
    if 'workspace' in arg or not arg.startswith('const '):
      return True
  return False


def _lib():
  import vtc_hip
  return vtc_hip, vtc_hip.load_library()


def test_header_is_parsed():
  decl = declarations()
  assert sorted(decl) == [
      'vtc_image_abi_version', 'vtc_img_assemble_patches',
      'vtc_img_downsample', 'vtc_img_filter_fd',
      'vtc_img_filter_fd_workspace_bytes', 'vtc_img_filter_sd',
      'vtc_img_filter_sd_workspace_bytes', 'vtc_img_tile_patches']
  assert needs_a_fence(decl['vtc_img_filter_fd'])
  assert needs_a_fence(decl['vtc_img_downsample'])
  assert not needs_a_fence(decl['vtc_img_filter_sd_workspace_bytes'])
  assert re.search(r'#define\s+VTC_IMAGE_ABI_VERSION\s+1\b', _code(HEADER))


def test_the_two_headers_do_not_overlap():
  main = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(MAIN_HEADER)))
  assert not main & set(declarations())


def test_binding_table_is_the_declared_surface():
  vtc_hip, lib = _lib()
  assert sorted(vtc_hip.IMAGE_SIGNATURES) == sorted(declarations())
  assert not set(vtc_hip.IMAGE_SIGNATURES) & set(vtc_hip.SIGNATURES)
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declarations().items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.IMAGE_SIGNATURES[name][1]) == count, name
    assert getattr(lib, name).argtypes == vtc_hip.IMAGE_SIGNATURES[name][1]
  assert lib.vtc_image_abi_version() == vtc_hip.IMAGE_ABI_VERSION == 1


def test_every_writing_entry_point_has_a_fenced_case():
  decl = declarations()
  fenced = set(c.entry for c in table.CASES)
  assert fenced <= set(decl), sorted(fenced - set(decl))
  missing = [name for name, args in sorted(decl.items())
             if needs_a_fence(args) and name not in fenced
             and name not in EXEMPT]
  assert not missing, 'no fenced case for: ' + ', '.join(missing)
  for name in EXEMPT:
    assert name in decl and name not in fenced, name
  ids = [c.id for c in table.CASES]
  assert len(ids) == len(set(ids))
  # both element types and both routes of the two-route entry points
  for stem in ('img_filter_fd-f32', 'img_filter_fd-u8',
               'img_filter_sd-general-f32', 'img_filter_sd-general-u8',
               'img_filter_sd-separable-f32', 'img_filter_sd-separable-u8',
               'img_tile_patches-f32', 'img_tile_patches-u8',
               'img_assemble_patches-disjoint-f32',
               'img_assemble_patches-disjoint-u8',
               'img_assemble_patches-ordered-f32',
               'img_assemble_patches-ordered-u8', 'img_downsample-f32',
               'img_downsample-u8'):
    assert any(i.startswith(stem) for i in ids), stem


def test_workspace_queries_are_host_only():
  _, lib = _lib()
  fd = lib.vtc_img_filter_fd_workspace_bytes
  # float64 planes and their half spectra, each piece rounded up to 256 bytes
  assert fd(2, 37, 53, 2, 40, 64) == 4 * 40 * 64 * 8 + 4 * 40 * 33 * 16
  assert fd(1, 37, 53, 1, 37, 53) == (
      -(-37 * 53 * 8 // 256) * 256 + -(-37 * 27 * 16 // 256) * 256)
  assert fd(2, 37, 53, 2, 36, 64) == 0 and fd(0, 37, 53, 2, 40, 64) == 0
  sd = lib.vtc_img_filter_sd_workspace_bytes
  assert sd(2, 37, 53, 2, 5, 3, 1) == 4 * 2 * 37 * 53 * 2
  assert sd(2, 37, 53, 2, 5, 3, 0) == 0
  assert sd(2, 37, 53, 2, 64, 3, 1) == 0 and sd(2, 37, 53, 2, 5, 54, 1) == 0


def _refused(lib, rc, status, *words):
  assert rc == status, (rc, lib.vtc_last_error())
  text = lib.vtc_last_error().decode()
  for word in words:
    assert word in text, text


def test_argument_errors_do_not_touch_the_gpu():
  """Null pointers, bad sizes, unknown element types and unsupported filter
  sizes come back before any HIP call: this runs with no device.  The
  non-null pointers are host integers that are never dereferenced."""
  vtc_hip, lib = _lib()
  p = ctypes.c_void_p(4096)
  q = ctypes.c_void_p(8192)
  inv, uns = ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED

  fd = lib.vtc_img_filter_fd
  _refused(lib, fd(None, F32, p, q, 1, 8, 8, 1, 8, 8, p, 1 << 20, None), inv,
           'vtc_img_filter_fd', 'null')
  _refused(lib, fd(p, F32, None, q, 1, 8, 8, 1, 8, 8, p, 1 << 20, None), inv,
           'null')
  _refused(lib, fd(p, F32, p, None, 1, 8, 8, 1, 8, 8, p, 1 << 20, None), inv,
           'null')
  _refused(lib, fd(p, F32, p, q, 0, 8, 8, 1, 8, 8, p, 1 << 20, None), inv,
           'shape')
  _refused(lib, fd(p, 7, p, q, 1, 8, 8, 1, 8, 8, p, 1 << 20, None), inv,
           'dtype')
  _refused(lib, fd(p, F32, p, q, 1, 8, 8, 1, 7, 8, p, 1 << 20, None), inv,
           'undersamples')
  _refused(lib, fd(p, F32, q, p, 1, 8, 8, 1, 8, 8, q, 1 << 20, None), inv,
           'alias')
  need = lib.vtc_img_filter_fd_workspace_bytes(1, 8, 8, 1, 8, 8)
  _refused(lib, fd(p, F32, p, q, 1, 8, 8, 1, 8, 8, p, need - 1, None),
           ERR_WORKSPACE, 'workspace')
  _refused(lib, fd(p, F32, p, q, 1, 8, 8, 1, 8, 8, None, need, None),
           ERR_WORKSPACE, 'workspace')

  sd = lib.vtc_img_filter_sd
  _refused(lib, sd(None, F32, p, None, None, q, 1, 8, 8, 1, 3, 3, None, 0,
                   None), inv, 'vtc_img_filter_sd', 'null')
  _refused(lib, sd(p, F32, None, None, None, q, 1, 8, 8, 1, 3, 3, None, 0,
                   None), inv, 'null')
  _refused(lib, sd(p, F32, None, p, None, q, 1, 8, 8, 1, 3, 3, None, 0, None),
           inv, 'null')
  _refused(lib, sd(p, F32, p, None, None, q, 1, 8, 8, 1, 0, 3, None, 0, None),
           inv, 'shape')
  _refused(lib, sd(p, 2, p, None, None, q, 1, 8, 8, 1, 3, 3, None, 0, None),
           inv, 'dtype')
  _refused(lib, sd(p, F32, p, None, None, q, 1, 80, 80, 1, 64, 3, None, 0,
                   None), uns, '63 taps')
  _refused(lib, sd(p, F32, p, None, None, q, 1, 8, 8, 1, 3, 9, None, 0, None),
           uns, 'no larger than the image')
  _refused(lib, sd(p, U8, None, p, p, q, 1, 8, 8, 1, 9, 3, p, 1 << 20, None),
           uns, 'no larger than the image')
  _refused(lib, sd(p, F32, None, p, p, q, 1, 8, 8, 1, 3, 3, p, 255, None),
           ERR_WORKSPACE, 'workspace')
  try:
    vtc_hip.check(uns, 'vtc_img_filter_sd')
  except NotImplementedError:
    pass
  else:
    raise AssertionError('VTC_ERR_UNSUPPORTED must raise NotImplementedError')

  tile = lib.vtc_img_tile_patches
  _refused(lib, tile(None, F32, q, 1, 8, 8, 1, 4, 4, None), inv,
           'vtc_img_tile_patches', 'null')
  _refused(lib, tile(p, F32, None, 1, 8, 8, 1, 4, 4, None), inv, 'null')
  _refused(lib, tile(p, F32, q, 1, 8, 8, 1, 9, 4, None), inv, 'sizes')
  _refused(lib, tile(p, F32, q, 1, 8, 8, 1, 4, 0, None), inv, 'sizes')
  _refused(lib, tile(p, 5, q, 1, 8, 8, 1, 4, 4, None), inv, 'dtype')

  asm = lib.vtc_img_assemble_patches
  _refused(lib, asm(None, F32, p, q, 4, 4, 4, 1, 8, 8, 1, None), inv,
           'vtc_img_assemble_patches', 'null')
  _refused(lib, asm(p, F32, None, q, 4, 4, 4, 1, 8, 8, 1, None), inv, 'null')
  _refused(lib, asm(p, F32, p, None, 4, 4, 4, 1, 8, 8, 0, None), inv, 'null')
  _refused(lib, asm(p, F32, p, q, 0, 4, 4, 1, 8, 8, 1, None), inv, 'sizes')
  _refused(lib, asm(p, F32, p, q, 4, 4, 4, 1, 3, 8, 1, None), inv, 'sizes')
  _refused(lib, asm(p, -1, p, q, 4, 4, 4, 1, 8, 8, 1, None), inv, 'dtype')

  down = lib.vtc_img_downsample
  _refused(lib, down(None, F32, q, 1, 8, 8, 1, 2, None), inv,
           'vtc_img_downsample', 'null')
  _refused(lib, down(p, F32, None, 1, 8, 8, 1, 2, None), inv, 'null')
  _refused(lib, down(p, F32, q, 1, 8, 8, 1, 0, None), inv, 'sizes')
  _refused(lib, down(p, F32, q, 1, 8, 0, 1, 2, None), inv, 'sizes')
  _refused(lib, down(p, 9, q, 1, 8, 8, 1, 2, None), inv, 'dtype')


def test_host_side_filter_builders():
  """numpy in, numpy out; the shapes and the few values that pin each."""
  import numpy as np
  from utils import image_processing as ip
  assert np.array_equal(ip.get_binomial_filter_1d(2), [0.5, 0.5])
  assert np.array_equal(ip.get_binomial_filter_1d(5),
                        np.array([1, 4, 6, 4, 1]) / 16.)
  b = ip.get_binomial_filter_2d(3, 4)
  assert b.shape == (3, 4) and abs(b.sum() - 1) < 1e-15
  gauss = ip.get_gaussian_filter_2d(1.5, (7, 4))
  assert gauss.shape == (7, 4) and abs(gauss.sum() - 1) < 1e-15
  assert gauss[3, 2] == gauss.max()          # coordinates -3..3 and -2..1
  raw = ip.get_gaussian_filter_2d(2.0, (5, 5), normalized=False)
  assert raw[2, 2] == 1.0 and abs(raw[2, 4] - np.exp(-0.5)) < 1e-15
  ramp = ip.get_whitening_ramp_filter((8, 6), norm_and_threshold=False)
  assert ramp.dtype == np.complex128 and ramp[0, 0] == 0
  assert abs(ramp[4, 3] - np.sqrt(0.5)) < 1e-15
  normed = ip.get_whitening_ramp_filter((8, 6))
  assert normed[0, 0] == 1e-5 and abs(normed).max() == 1.0
  lp = ip.get_low_pass_filter((8, 6), {'shape': 'exponential', 'cutoff': 0.5,
                                       'order': 4.0})
  assert lp[0, 0] == 1.0 and lp[4, 3] == 1e-3
  try:
    ip.get_low_pass_filter((8, 6), {'shape': 'box'})
  except KeyError:
    pass
  else:
    raise AssertionError('unknown filter shape must raise KeyError')
  f = ip.center_surround_filter((16, 12, 3), {'low': 0.0, 'high': 0.8})
  assert f.shape == (16, 12) and f.dtype == np.complex128
  assert abs(f).max() == 1.0 and f[0, 0] == 1e-3 and abs(f).min() == 1e-3
  plain = ip.center_surround_filter((16, 12), {'low': 0.1, 'high': 0.8},
                                    norm_and_threshold=False)
  assert abs(plain[0, 0] - 0.1) < 1e-15
