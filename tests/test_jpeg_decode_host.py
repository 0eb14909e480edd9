"""The fourth header, include/vtc_decode.h, held to what tests/
test_jpeg_host.py asks of the third: DECODE_SIGNATURES is exactly the declared
surface and shares no name with the other three, the library exports it, the
four version numbers, the workspace query term for term, bad arguments
answered before any device work, and the host half of the decoder in
utils/jpeg.py.  No GPU needed."""
import ctypes
import pathlib
import re

import pytest

import test_jpeg_decode_abi_gpu as table

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'vtc_decode.h'
OTHER_HEADERS = [REPO / 'include' / name
                 for name in ('vtc_hip.h', 'vtc_image.h', 'vtc_codec.h')]

OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, 1, 2, 3


def _code(path):
  return re.sub(r'/\*.*?\*/', '', path.read_text(), flags=re.S)


def declarations():
  """name -> argument text of every function include/vtc_decode.h declares."""
  return {m.group(1): m.group(2)
          for m in re.finditer(r'\b(vtc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;',
                               _code(HEADER))}


def _lib():
  import vtc_hip
  return vtc_hip, vtc_hip.load_library()


def test_header_is_parsed():
  assert sorted(declarations()) == [
      'vtc_decode_abi_version', 'vtc_jpeg_unpack',
      'vtc_jpeg_unpack_workspace_bytes']
  assert re.search(r'#define\s+VTC_DECODE_ABI_VERSION\s+1\b', _code(HEADER))


def test_the_four_headers_do_not_overlap():
  for other in OTHER_HEADERS:
    names = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(other)))
    assert names and not names & set(declarations()), other.name


def test_binding_table_is_the_declared_surface():
  vtc_hip, lib = _lib()
  assert sorted(vtc_hip.DECODE_SIGNATURES) == sorted(declarations())
  for other in (vtc_hip.SIGNATURES, vtc_hip.IMAGE_SIGNATURES,
                vtc_hip.CODEC_SIGNATURES):
    assert not set(vtc_hip.DECODE_SIGNATURES) & set(other)
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declarations().items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.DECODE_SIGNATURES[name][1]) == count, name
    assert getattr(lib, name).argtypes == vtc_hip.DECODE_SIGNATURES[name][1]
  assert lib.vtc_decode_abi_version() == vtc_hip.DECODE_ABI_VERSION == 1
  # the other three versions stay where they were
  assert lib.vtc_abi_version() == 4
  assert lib.vtc_image_abi_version() == 1
  assert lib.vtc_codec_abi_version() == 1


def test_the_writing_entry_point_has_fenced_cases():
  assert set(c.entry for c in table.CASES) == {'vtc_jpeg_unpack'}
  ids = [c.id for c in table.CASES]
  assert len(ids) == len(set(ids)) and len(ids) >= 2


def test_workspace_query_is_stated_term_for_term():
  """272 sorted codewords as uint64, their 272 uint16 meta words, two
  first-level lookups of 2^10 uint16 entries, int32[4]; each array rounded up
  to 256 bytes."""
  _, lib = _lib()

  def padded(nbytes):
    return -(-nbytes // 256) * 256

  assert lib.vtc_jpeg_unpack_workspace_bytes() == (
      padded(272 * 8) + padded(272 * 2) + padded(2 * 1024 * 2) + padded(4 * 4))
  assert lib.vtc_jpeg_unpack_workspace_bytes() == 7424


def _refused(lib, rc, status, *words):
  assert rc == status, (rc, lib.vtc_last_error())
  text = lib.vtc_last_error().decode()
  for word in words:
    assert word in text, text


def test_argument_errors_do_not_touch_the_gpu():
  """Every null pointer, d = 0, s of 0 or 4097, an empty buffer and a short
  workspace come back before any HIP call: this runs with no device.  The
  non-null pointers are host integers that are never dereferenced."""
  _, lib = _lib()
  p, q, r = (ctypes.c_void_p(v) for v in (4096, 8192, 16384))
  need = lib.vtc_jpeg_unpack_workspace_bytes()
  unpack = lib.vtc_jpeg_unpack
  #        packed bytes offsets d s  ac_code ac_len dc_code dc_len levels status
  good = [p, 100, q, 3, 64, r, p, q, r, p, q, r, need, None]
  inv = ERR_INVALID_ARGUMENT
  for position in (0, 2, 5, 6, 7, 8, 9, 10):
    args = list(good)
    args[position] = None
    _refused(lib, unpack(*args), inv, 'vtc_jpeg_unpack', 'null')
  for position, value, word in ((3, 0, 'd = 0'), (3, -1, 'd = -1'),
                                (4, 0, 's = 0'), (4, 4097, 's = 4097'),
                                (1, 0, 'packed_bytes = 0')):
    args = list(good)
    args[position] = value
    _refused(lib, unpack(*args), inv, 'vtc_jpeg_unpack', word)
  args = list(good)
  args[12] = need - 1
  _refused(lib, unpack(*args), ERR_WORKSPACE, 'workspace',
           '%d bytes, %d needed' % (need - 1, need))
  args = list(good)
  args[11] = None
  _refused(lib, unpack(*args), ERR_WORKSPACE, 'workspace')


def test_error_mapping_of_the_python_layer():
  import torch
  import vtc_hip
  from utils import jpeg
  table_ac = {'00': '0', '01': '10', '11': '11'}
  table_dc = {'-': '0', '1': '1'}
  packed = torch.zeros(4, dtype=torch.uint8)
  offsets = torch.zeros(2, dtype=torch.int64)
  with pytest.raises(vtc_hip.VtcHipError):
    jpeg.unpack_streams(packed, offsets, 8, table_ac, table_dc)
  with pytest.raises(TypeError):
    jpeg.unpack_streams([0, 0], offsets, 8, table_ac, table_dc)
  with pytest.raises(vtc_hip.VtcHipError):
    jpeg.decode_patches(packed, offsets, torch.eye(8), [1.] * 8, 1.0,
                        (table_ac, table_dc))
  with pytest.raises(TypeError):
    jpeg.parse_jpg_binary_stream('0120', 8, [0] * 8, table_ac, table_dc)
  # the existing table_arrays is what refuses a codeword of over 64 bits
  with pytest.raises(NotImplementedError):
    jpeg.table_arrays({'00': '0', '01': '1' + '0' * 64}, jpeg._AC_BYTE, 256)
  # and a table that cannot be decoded is refused before any tensor is looked
  # at
  with pytest.raises(ValueError):
    jpeg.unpack_streams(packed, offsets, 8, {'00': '0', '01': '01'}, table_dc)


def test_host_prefix_check():
  from utils import jpeg
  jpeg.check_prefix_free({})
  jpeg.check_prefix_free({'00': '0'})
  jpeg.check_prefix_free({'00': '00', '01': '01', '02': '10', 'f0': '110',
                          '11': '111'})
  with pytest.raises(ValueError) as caught:
    jpeg.check_prefix_free({'00': '00', '01': '101', '02': '10', 'f0': '11'})
  assert "'02'" in str(caught.value) and "'01'" in str(caught.value)
  assert 'is a prefix of' in str(caught.value)
  with pytest.raises(ValueError) as caught:
    jpeg.check_prefix_free({'00': '00', '21': '011', '02': '10', 'a3': '011'})
  assert "'21'" in str(caught.value) and "'a3'" in str(caught.value)
  assert 'equals' in str(caught.value)
  # not neighbours as symbols, neighbours as words; the DC spellings too
  with pytest.raises(ValueError) as caught:
    jpeg.check_prefix_free({'-': '1', '1': '00', '2': '010', 'a': '0110',
                            '3': '01'})
  assert "'3'" in str(caught.value)
