"""The tenth header, include/vtc_index_decode.h, held to what
tests/test_index_code_host.py asks of the ninth: INDEX_DECODE_SIGNATURES is
exactly the declared surface and shares no name with the other nine tables,
whose versions stay where they were; the library exports it; bad arguments are
answered before any device work; the workspace query is host-only.  Then the
restatement of tests/index_decode_data.py against hand-worked cases.  No GPU
needed."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import index_code_data as data
import index_decode_data as truth

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'vtc_index_decode.h'
OTHER_HEADERS = [REPO / 'include' / name
                 for name in ('vtc_hip.h', 'vtc_image.h', 'vtc_codec.h',
                              'vtc_decode.h', 'vtc_quality.h', 'vtc_stats.h',
                              'vtc_quant.h', 'vtc_vq.h', 'vtc_index_code.h')]

OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, 1, 2, 3


def _code(path):
  return re.sub(r'/\*.*?\*/', '', path.read_text(), flags=re.S)


def declarations():
  """name -> argument text of every function the header declares."""
  return {m.group(1): m.group(2)
          for m in re.finditer(r'\b(vtc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;',
                               _code(HEADER))}


def _lib():
  import vtc_hip
  return vtc_hip, vtc_hip.load_library()


def test_header_is_parsed():
  assert sorted(declarations()) == [
      'vtc_index_code_unpack', 'vtc_index_code_unpack_workspace_bytes',
      'vtc_index_decode_abi_version']
  code = _code(HEADER)
  assert re.search(r'#define\s+VTC_INDEX_DECODE_ABI_VERSION\s+1\b', code)
  assert re.search(r'#define\s+VTC_INDEX_DECODE_LOOKUP_BITS\s+%d\b'
                   % truth.LOOKUP_BITS, code)
  assert '#include "vtc_index_code.h"' in code


def test_the_ten_headers_do_not_overlap():
  for other in OTHER_HEADERS:
    names = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(other)))
    assert names and not names & set(declarations()), other.name


def test_binding_table_is_the_declared_surface():
  vtc_hip, lib = _lib()
  assert sorted(vtc_hip.INDEX_DECODE_SIGNATURES) == sorted(declarations())
  for other in (vtc_hip.SIGNATURES, vtc_hip.IMAGE_SIGNATURES,
                vtc_hip.CODEC_SIGNATURES, vtc_hip.DECODE_SIGNATURES,
                vtc_hip.QUALITY_SIGNATURES, vtc_hip.STATS_SIGNATURES,
                vtc_hip.QUANT_SIGNATURES, vtc_hip.VQ_SIGNATURES,
                vtc_hip.INDEX_CODE_SIGNATURES):
    assert not set(vtc_hip.INDEX_DECODE_SIGNATURES) & set(other)
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declarations().items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.INDEX_DECODE_SIGNATURES[name][1]) == count, name
    assert getattr(lib, name).argtypes == (
        vtc_hip.INDEX_DECODE_SIGNATURES[name][1])
  assert (lib.vtc_index_decode_abi_version() ==
          vtc_hip.INDEX_DECODE_ABI_VERSION == 1)
  assert vtc_hip.INDEX_DECODE_LOOKUP_BITS == truth.LOOKUP_BITS
  # the other nine stay where they were
  assert (lib.vtc_abi_version(), lib.vtc_image_abi_version(),
          lib.vtc_codec_abi_version(), lib.vtc_decode_abi_version(),
          lib.vtc_quality_abi_version(), lib.vtc_stats_abi_version(),
          lib.vtc_quant_abi_version(), lib.vtc_vq_abi_version(),
          lib.vtc_index_code_abi_version()) == (4, 1, 1, 1, 1, 1, 1, 1, 1)
  assert len(vtc_hip.INDEX_CODE_SIGNATURES) == 3
  assert len(vtc_hip.DECODE_SIGNATURES) == 3


def _refused(lib, rc, status, *words):
  assert rc == status, (rc, lib.vtc_last_error())
  text = lib.vtc_last_error().decode()
  for word in words:
    assert word in text, text


def test_argument_errors_do_not_touch_the_gpu():
  """Null pointers, bad sizes, unsupported sizes and a short workspace, one
  argument at a time.  The non-null pointers are host integers that are never
  dereferenced: this runs with no device."""
  _, lib = _lib()
  p = [ctypes.c_void_p(v << 20) for v in range(1, 12)]
  who = 'vtc_index_code_unpack'
  need = lib.vtc_index_code_unpack_workspace_bytes(42, 40)
  assert need > 0
  #       packed bytes offsets b   m   code  len  kmax indices rows  status
  good = [p[0], 1000, p[1], 257, 42, p[2], p[3], 40, p[4], p[5], p[6],
          p[7], need, None]     # workspace, its bytes, stream
  for position in (0, 2, 5, 6, 8, 9, 10):
    args = list(good)
    args[position] = None
    _refused(lib, lib.vtc_index_code_unpack(*args), ERR_INVALID_ARGUMENT, who,
             'null')
  for position, value, word in ((3, 0, 'b = 0'), (3, -3, 'b = -3'),
                                (4, 0, 'm = 0'), (4, -1, 'm = -1'),
                                (7, 0, 'kmax = 0'), (7, -7, 'kmax = -7'),
                                (1, -1, 'packed_bytes = -1'),
                                (1, 1 << 59, 'packed_bytes')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_index_code_unpack(*args), ERR_INVALID_ARGUMENT, who,
             word)
  for position, value, word in ((4, 4097, 'm = 4097'),
                                (7, 4097, 'kmax = 4097'),
                                (3, 1 << 44, 'too many rows')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_index_code_unpack(*args), ERR_UNSUPPORTED, who, word)
  # the workspace: null, one byte short, none
  for pointer, nbytes in ((None, need), (p[7], need - 1), (p[7], 0)):
    args = list(good)
    args[11], args[12] = pointer, nbytes
    _refused(lib, lib.vtc_index_code_unpack(*args), ERR_WORKSPACE, who,
             'workspace', '%d needed' % need)


def test_workspace_query():
  """Host-only (no device here), monotone in m and kmax, the documented sum,
  0 for the sizes the call refuses."""
  _, lib = _lib()
  query = lib.vtc_index_code_unpack_workspace_bytes

  def up(v):
    return -(-v // 256) * 256

  for m, kmax in ((1, 1), (1, 4096), (42, 1024), (5, 300), (4096, 4),
                  (4096, 4096)):
    want = (up(8 * m * kmax) + up(4 * m * kmax) +
            up(4 * (m << truth.LOOKUP_BITS)) + up(4 * m) + up(4))
    assert query(m, kmax) == want, (m, kmax)
  sizes = (1, 2, 63, 64, 65, 300, 1024, 4095, 4096)
  for a, b in zip(sizes, sizes[1:]):
    assert query(a, 40) <= query(b, 40) and query(42, a) <= query(42, b)
    assert query(a, a) < query(b, b)
  for m, kmax in ((0, 40), (-1, 40), (4097, 40), (42, 0), (42, -5),
                  (42, 4097)):
    assert query(m, kmax) == 0, (m, kmax)


def test_cpu_tensors_are_refused():
  import torch
  import vtc_hip
  from utils import index_coding
  from utils import quantization
  packed = torch.zeros(4, dtype=torch.uint8)
  offsets = torch.zeros(3, dtype=torch.int64)
  tables = [{0: '0', 1: '1'}, {0: ''}]
  with pytest.raises(vtc_hip.VtcHipError):
    index_coding.unpack_index_streams(packed, offsets, tables)
  with pytest.raises(vtc_hip.VtcHipError):
    quantization.decode_codes(packed, offsets, tables, np.zeros((2, 2)))
  # a table that is not prefix-free is answered first, before any device work
  for bad in ({0: '01', 1: '01'}, {0: '0', 1: '01'}, {0: '', 1: '0'}):
    with pytest.raises(ValueError):
      index_coding.unpack_index_streams(packed, offsets, [tables[0], bad])
  with pytest.raises(TypeError):
    index_coding.parse_index_stream('0120', tables)


# -------------------------------------------------------------- restatement
def test_restatement_on_a_hand_worked_case():
  """The ['100', '01', '11', '0'] example of tests/test_index_code_host.py,
  read back.  Rows 2 and 3 were packed from entries their tables lack and miss
  their third codeword: row 2 reads the gap bit behind it instead, row 3 has
  no bit left."""
  tables = [{0: '0', 1: '10', 2: '11'}, {0: ''}, {0: '1', 3: '0'}]
  offsets = np.array([3, 6, 13, 16, 17], np.int64)
  #                    ...100 01..... 11 0
  bits = '000100010000011000000000'
  packed = np.packbits(np.array([c == '1' for c in bits], np.uint8))
  assert truth.bit_string(packed) == bits
  indices, rows, malformed, bad = truth.decode(packed, offsets, tables, 4)
  assert bad is None and malformed == [3]
  assert indices.tolist() == [[1, 0, 3], [0, 0, 0], [2, 0, 3], [0, 0, -1]]
  assert rows.tolist() == [3, 2, 3, 1]
  assert truth.status(malformed, bad) == [1, 4, 0]
  # the spans of rows 0 and 1 are 3 and 7 bits: row 1 leaves 5 unread, which
  # is no fault
  assert (np.diff(offsets) - rows).tolist() == [0, 5, 0, 0]

  # two bytes short: row 1 ends with the buffer, rows 2 and 3 start past it
  indices, rows, malformed, bad = truth.decode(packed[:1], offsets, tables, 4)
  assert malformed == [2, 3] and truth.status(malformed, bad) == [2, 3, 0]
  assert indices.tolist() == [[1, 0, 3], [0, 0, 0], [-1, -1, -1],
                              [-1, -1, -1]]
  assert rows.tolist() == [3, 2, 0, 0]
  # a row cut by its end, a decreasing and a negative offset
  indices, rows, malformed, _ = truth.decode(
      packed, np.array([3, 5, 13, 12, 17]), tables, 4)
  assert malformed == [0, 2] and indices[0].tolist() == [1, 0, -1]
  assert indices[1].tolist() == [0, 0, 3] and rows.tolist() == [2, 2, 0, 2]
  indices, rows, malformed, _ = truth.decode(
      packed, np.array([-1, 6]), tables, 4)
  assert malformed == [0] and rows.tolist() == [0]
  # no codeword matches: '11' under an incomplete table; a column of none
  partial = [{0: '00', 1: '01', 2: '10'}]
  indices, rows, malformed, _ = truth.decode(
      np.array([0b00111000], np.uint8), np.array([0, 2, 4, 6]), partial, 3)
  assert indices.tolist() == [[0], [-1], [2]] and malformed == [1]
  assert rows.tolist() == [2, 0, 2]
  indices, rows, malformed, _ = truth.decode(
      np.array([0b01000000], np.uint8), np.array([0, 2]),
      [{0: '0', 1: '1'}, {}, {0: '0', 1: '1'}], 2)
  assert indices.tolist() == [[0, -1, -1]] and rows.tolist() == [1]
  # the empty codeword consumes nothing, with no bytes at all
  indices, rows, malformed, bad = truth.decode(
      np.zeros(0, np.uint8), np.zeros(5, np.int64), [{0: ''}], 1)
  assert indices.tolist() == [[0]] * 4 and malformed == [] and bad is None
  assert rows.tolist() == [0] * 4


def test_restatement_of_the_table_check():
  kmax = 4
  good = {0: '0', 1: '10', 2: '11'}
  assert truth.first_bad_position([good, {0: ''}, good], kmax) is None
  equal = {0: '0', 1: '10', 2: '10'}
  assert truth.first_bad_position([good, equal], kmax) == kmax + 1
  prefix = {0: '00', 1: '1', 2: '10'}
  assert truth.first_bad_position([good, good, prefix], kmax) == 2 * kmax + 1
  assert truth.first_bad_position([{0: '', 1: '0'}], kmax) == 0
  assert truth.first_bad_position([{1: '', 0: '0'}], kmax) == 1
  indices, rows, malformed, bad = truth.decode(
      np.array([0], np.uint8), np.array([0, 1, 2]), [good, equal], kmax)
  assert (indices == -1).all() and (rows == 0).all() and malformed == []
  assert truth.status(malformed, bad) == [0, 0, kmax + 2]


def test_restatement_reads_back_the_shared_cases():
  """What data.image writes for the shared shapes decodes to the shared
  indices, behind every lead."""
  assert len(truth.SHAPES) == 13 and truth.SHAPES[-1] == (7, 5, 300)
  for shape in truth.SHAPES:
    tables, _ = data.case_tables(*shape)
    host = data.case_indices(*shape)
    for lead in data.LEADS:
      packed, offsets = truth.case_stream(shape, lead)
      indices, rows, malformed, bad = truth.decode(packed, offsets, tables,
                                                   shape[2])
      assert bad is None and malformed == []
      assert np.array_equal(indices, host)
      assert np.array_equal(rows, data.row_bits(host, tables))


def test_the_long_table_straddles_the_lookup():
  table = truth.long_table()
  lengths = sorted(len(word) for word in table.values())
  assert lengths == list(range(1, 65)) + [64]
  assert {truth.LOOKUP_BITS, truth.LOOKUP_BITS + 1, 57, 64} <= set(lengths)
