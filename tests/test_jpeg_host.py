"""The third header, include/vtc_codec.h, held to what tests/
test_image_abi_host.py asks of the second: CODEC_SIGNATURES is exactly the
declared surface, the library exports it, every writing entry point has a
fenced row in tests/test_jpeg_abi_gpu.py, bad arguments are answered before
any device work.  And the host half of utils/jpeg.py and utils/
matrix_zigzag.py against tests/golden/jpeg.npz (tools/make_jpeg_golden.py: the
reference's own results).  No GPU needed."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import helpers
import test_jpeg_abi_gpu as table

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'vtc_codec.h'
OTHER_HEADERS = [REPO / 'include' / 'vtc_hip.h',
                 REPO / 'include' / 'vtc_image.h']

EXEMPT = {
    'vtc_codec_abi_version': 'returns an integer',
}

OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, 1, 2, 3


def _code(path):
  return re.sub(r'/\*.*?\*/', '', path.read_text(), flags=re.S)


def declarations():
  """name -> argument text of every function include/vtc_codec.h declares."""
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


@pytest.fixture(scope='module')
def golden():
  return helpers.load('jpeg')


def _strings(array):
  return [b.decode('ascii') for b in array.tolist()]


# ------------------------------------------------------------------ the ABI
def test_header_is_parsed():
  decl = declarations()
  assert sorted(decl) == [
      'vtc_codec_abi_version', 'vtc_jpeg_bit_offsets',
      'vtc_jpeg_bit_offsets_workspace_bytes', 'vtc_jpeg_dequantize',
      'vtc_jpeg_pack', 'vtc_jpeg_quantize', 'vtc_jpeg_stream_bits',
      'vtc_jpeg_symbol_counts']
  assert needs_a_fence(decl['vtc_jpeg_pack'])
  assert not needs_a_fence(decl['vtc_jpeg_bit_offsets_workspace_bytes'])
  assert re.search(r'#define\s+VTC_CODEC_ABI_VERSION\s+1\b', _code(HEADER))
  assert re.search(r'#define\s+VTC_JPEG_MAX_S\s+4096\b', _code(HEADER))


def test_the_three_headers_do_not_overlap():
  for other in OTHER_HEADERS:
    names = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(other)))
    assert not names & set(declarations()), other.name


def test_binding_table_is_the_declared_surface():
  vtc_hip, lib = _lib()
  assert sorted(vtc_hip.CODEC_SIGNATURES) == sorted(declarations())
  assert not set(vtc_hip.CODEC_SIGNATURES) & set(vtc_hip.SIGNATURES)
  assert not set(vtc_hip.CODEC_SIGNATURES) & set(vtc_hip.IMAGE_SIGNATURES)
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declarations().items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.CODEC_SIGNATURES[name][1]) == count, name
    assert getattr(lib, name).argtypes == vtc_hip.CODEC_SIGNATURES[name][1]
  assert lib.vtc_codec_abi_version() == vtc_hip.CODEC_ABI_VERSION == 1
  # the other two versions stay where they were
  assert lib.vtc_abi_version() == 4 and lib.vtc_image_abi_version() == 1


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
  for stem in ('jpeg_quantize-identity', 'jpeg_quantize-order',
               'jpeg_dequantize-identity', 'jpeg_dequantize-order',
               'jpeg_symbol_counts', 'jpeg_stream_bits', 'jpeg_bit_offsets',
               'jpeg_pack-exact', 'jpeg_pack-short'):
    assert any(i.startswith(stem) for i in ids), stem


def test_workspace_query_is_stated_term_for_term():
  """One int64 per tile of 2048 rows, the array rounded up to 256 bytes."""
  _, lib = _lib()
  query = lib.vtc_jpeg_bit_offsets_workspace_bytes
  for d in (1, 3, 2048, 2049, 5000, 1 << 20, (1 << 20) + 1):
    tiles = -(-d // 2048)
    assert query(d) == -(-tiles * 8 // 256) * 256, d
  assert query(0) == 0 and query(-5) == 0


def _refused(lib, rc, status, *words):
  assert rc == status, (rc, lib.vtc_last_error())
  text = lib.vtc_last_error().decode()
  for word in words:
    assert word in text, text


def test_argument_errors_do_not_touch_the_gpu():
  """Null pointers, s of 0 or 4097, negative d and a short workspace come back
  before any HIP call: this runs with no device.  The non-null pointers are
  host integers that are never dereferenced."""
  _, lib = _lib()
  p, q, r = (ctypes.c_void_p(v) for v in (4096, 8192, 16384))
  inv = ERR_INVALID_ARGUMENT

  for name in ('vtc_jpeg_quantize', 'vtc_jpeg_dequantize'):
    fn = getattr(lib, name)
    _refused(lib, fn(None, p, None, q, 3, 64, None), inv, name, 'null')
    _refused(lib, fn(p, None, None, q, 3, 64, None), inv, name, 'null')
    _refused(lib, fn(p, q, None, None, 3, 64, None), inv, name, 'null')
    _refused(lib, fn(p, q, None, r, 3, 0, None), inv, name, 's = 0')
    _refused(lib, fn(p, q, None, r, 3, 4097, None), inv, name, 's = 4097')
    _refused(lib, fn(p, q, None, r, -1, 64, None), inv, name, 'd = -1')
    _refused(lib, fn(p, q, None, r, 0, 64, None), inv, name, 'd = 0')

  counts = lib.vtc_jpeg_symbol_counts
  _refused(lib, counts(None, 3, 64, p, q, r, None), inv,
           'vtc_jpeg_symbol_counts', 'null')
  _refused(lib, counts(p, 3, 64, None, q, r, None), inv, 'null')
  _refused(lib, counts(p, 3, 64, q, None, r, None), inv, 'null')
  _refused(lib, counts(p, 3, 64, q, r, None, None), inv, 'null')
  _refused(lib, counts(p, 3, 0, q, r, p, None), inv, 's = 0')
  _refused(lib, counts(p, 3, 4097, q, r, p, None), inv, 's = 4097')
  _refused(lib, counts(p, -2, 64, q, r, p, None), inv, 'd = -2')

  bits = lib.vtc_jpeg_stream_bits
  _refused(lib, bits(None, 3, 64, p, q, r, p, None), inv,
           'vtc_jpeg_stream_bits', 'null')
  _refused(lib, bits(p, 3, 64, None, q, r, p, None), inv, 'null')
  _refused(lib, bits(p, 3, 64, q, None, r, p, None), inv, 'null')
  _refused(lib, bits(p, 3, 64, q, r, None, p, None), inv, 'null')
  _refused(lib, bits(p, 3, 64, q, r, p, None, None), inv, 'null')
  _refused(lib, bits(p, 3, 0, q, r, p, q, None), inv, 's = 0')
  _refused(lib, bits(p, 3, 4097, q, r, p, q, None), inv, 's = 4097')
  _refused(lib, bits(p, -1, 64, q, r, p, q, None), inv, 'd = -1')

  offsets = lib.vtc_jpeg_bit_offsets
  need = lib.vtc_jpeg_bit_offsets_workspace_bytes(5000)
  assert need == 256
  _refused(lib, offsets(None, 5000, q, r, need, None), inv,
           'vtc_jpeg_bit_offsets', 'null')
  _refused(lib, offsets(p, 5000, None, r, need, None), inv, 'null')
  _refused(lib, offsets(p, -1, q, r, need, None), inv, 'd = -1')
  _refused(lib, offsets(p, 5000, q, r, need - 1, None), ERR_WORKSPACE,
           'workspace', '255 bytes, 256 needed')
  _refused(lib, offsets(p, 5000, q, None, need, None), ERR_WORKSPACE,
           'workspace')

  pack = lib.vtc_jpeg_pack
  good = [p, 3, 64, q, r, q, r, p, q, 100, r, None]
  for position in (0, 3, 4, 5, 6, 7, 8, 10):
    args = list(good)
    args[position] = None
    _refused(lib, pack(*args), inv, 'vtc_jpeg_pack', 'null')
  for position, value, word in ((2, 0, 's = 0'), (2, 4097, 's = 4097'),
                                (1, -1, 'd = -1'), (9, 0, 'out_bytes = 0')):
    args = list(good)
    args[position] = value
    _refused(lib, pack(*args), inv, 'vtc_jpeg_pack', word)


def test_error_mapping_of_the_python_layer():
  import torch
  import vtc_hip
  from utils import jpeg
  with pytest.raises(vtc_hip.VtcHipError):
    jpeg.symbol_counts(torch.zeros(2, 8, dtype=torch.int32))
  with pytest.raises(vtc_hip.VtcHipError):
    jpeg.quantize(torch.zeros(2, 8), np.ones(8))
  with pytest.raises(vtc_hip.VtcHipError):
    jpeg.generate_ac_dc_huffman_tables(torch.zeros(2, 8, dtype=torch.int64),
                                       np.zeros(8))
  with pytest.raises(NotImplementedError):
    jpeg.table_arrays({'00': '0' * 65}, jpeg._AC_BYTE, 256)
  code, length = jpeg.table_arrays({'00': '1' * 64, 'f0': '01'},
                                   jpeg._AC_BYTE, 256)
  assert int(code[0]) == 2 ** 64 - 1 and length[0] == 64
  assert int(code[0xF0]) == 1 and length[0xF0] == 2 and length[1] == 0


# ------------------------------------------------------------- host numerics
@pytest.mark.parametrize('shape', [(8, 8), (3, 5), (1, 7), (16, 16)])
def test_zigzag_equals_the_reference(golden, shape):
  from utils import matrix_zigzag
  tag = '%dx%d' % shape
  matrix = golden['zigzag_in_' + tag]
  scan = matrix_zigzag.zigzag(matrix)
  assert scan.dtype == np.float64 and scan.shape == (shape[0] * shape[1],)
  assert np.array_equal(scan, golden['zigzag_out_' + tag])
  back = matrix_zigzag.inverse_zigzag(scan, *shape)
  assert back.dtype == np.float64 and back.shape == shape
  assert np.array_equal(back, golden['zigzag_back_' + tag])
  # the inverse undoes the forward scan: at every position the scan visits
  # (all of them, except where the reference's walk leaves a shape such as
  # 3 x 5 early -- utils/matrix_zigzag.py), and scanning again gives the scan
  visited = matrix_zigzag.scan_positions(*shape)
  assert len(set(visited)) == len(visited)
  for v, h in visited:
    assert back[v, h] == matrix[v, h]
  if shape != (3, 5):
    assert len(visited) == matrix.size and np.array_equal(back, matrix)
  else:
    assert len(visited) == 12
  assert np.array_equal(matrix_zigzag.zigzag(back), scan)


def test_scan_order_is_the_zigzag_as_indices():
  from utils import matrix_zigzag
  order = matrix_zigzag.scan_order(8, 8)
  assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(64))
  assert order[:6].tolist() == [0, 1, 8, 16, 9, 2]
  assert np.array_equal(matrix_zigzag.zigzag(np.arange(64).reshape(8, 8)),
                        order)


def test_binwidths_equal_the_reference(golden):
  from utils import jpeg
  widths = jpeg.get_jpeg_quant_hifi_binwidths()
  assert widths.dtype == np.float64
  assert np.array_equal(widths, golden['binwidths'])
  assert widths[:4].tolist() == [16., 11., 12., 14.] and widths[-1] == 99.


def _table(golden, kind, tag):
  return list(zip(_strings(golden['table_%s_symbols_%s' % (kind, tag)]),
                  _strings(golden['table_%s_codes_%s' % (kind, tag)])))


def test_huffman_table_with_many_ties(golden):
  from utils import jpeg
  counts = dict(zip(_strings(golden['ties_counts_symbols']),
                    golden['ties_counts_weights'].tolist()))
  assert sum(1 for w in counts.values() if w == 1) > 100
  ours = jpeg.compute_huffman_table(counts)
  want = list(zip(_strings(golden['ties_table_symbols']),
                  _strings(golden['ties_table_codes'])))
  assert list(ours.items()) == want


@pytest.mark.parametrize('tag', ['1', '17', '64', '300', 'b257', 'b5000'])
def test_huffman_tables_from_the_fixtures_counts(golden, tag):
  """The reference's symbols, counted on the host, give the reference's
  tables string for string and in the reference's order."""
  from utils import jpeg
  if tag == 'b5000':
    ac, dc = golden['counts_ac_b5000'], golden['counts_dc_b5000']
  else:
    ac = np.bincount(golden['ac_' + tag], minlength=256)
    dc = np.bincount(golden['dc_' + tag], minlength=16)
  table_ac, table_dc = jpeg.tables_from_counts(ac, dc)
  assert list(table_ac.items()) == _table(golden, 'ac', tag)
  assert list(table_dc.items()) == _table(golden, 'dc', tag)


def test_value_bits_and_spellings():
  from utils import jpeg
  assert jpeg.jpg_coeff_to_binstr(0) == ''
  assert jpeg.jpg_coeff_to_binstr(5) == '101'
  assert jpeg.jpg_coeff_to_binstr(-5) == '010'
  assert jpeg.jpg_coeff_to_binstr(np.int32(-1)) == '0'
  assert jpeg.jpg_coeff_to_binstr(-32767) == '0' * 15
  assert jpeg.ac_symbol(0xF0) == 'f0' and jpeg.ac_symbol(0x0A) == '0a'
  assert jpeg.dc_symbol(0) == '-' and jpeg.dc_symbol(11) == 'b'


def test_the_constructed_rows_are_in_the_fixture(golden):
  """The fixture holds what the module text lists (read on the host)."""
  for s in golden['lengths'].tolist():
    levels = golden['levels_%d' % s]
    assert (levels == 0).all(1).any()
    assert ((levels[:, 0] != 0) & (levels[:, 1:] == 0).all(1)).any()
    assert (levels[:, s - 1] != 0).any()
    seen = set(np.unique(levels).tolist())
    for k in range(15):
      for m in ((1 << k) - 1, 1 << k):
        assert m in seen and -m in seen, (s, m)
  big = golden['levels_300']
  gaps = set()
  for row in big:
    nz = np.flatnonzero(row[1:]) + 1
    gaps |= set(np.diff(np.concatenate([[0], nz])) - 1)
  assert {15, 16, 17, 31, 32, 33, 255} <= gaps
  l130 = golden['levels_130']
  assert any(r[3] and r[129] and np.count_nonzero(r) == 2 for r in l130)
  assert any(r[60] and r[70] and np.count_nonzero(r) == 2 for r in l130)
