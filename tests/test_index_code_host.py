"""The ninth header, include/vtc_index_code.h, held to what
tests/test_vq_host.py asks of the eighth: INDEX_CODE_SIGNATURES is exactly the
declared surface and shares no name with the other eight tables, whose
versions stay where they were; the library exports it; bad arguments are
answered before any device work.  Then the host half of utils.index_coding:
the Huffman tables against an independent cost computation, and the
restatement of tests/index_code_data.py against hand-worked cases.  No GPU
needed."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import index_code_data as data

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'vtc_index_code.h'
OTHER_HEADERS = [REPO / 'include' / name
                 for name in ('vtc_hip.h', 'vtc_image.h', 'vtc_codec.h',
                              'vtc_decode.h', 'vtc_quality.h', 'vtc_stats.h',
                              'vtc_quant.h', 'vtc_vq.h')]

OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = 0, 1, 2


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
      'vtc_index_code_abi_version', 'vtc_index_code_bits',
      'vtc_index_code_pack']
  code = _code(HEADER)
  for name, value in (('ABI_VERSION', 1), ('ABSENT', data.ABSENT),
                      ('MAX_COLUMNS', data.MAX_COLUMNS),
                      ('MAX_SYMBOLS', data.MAX_SYMBOLS)):
    assert re.search(r'#define\s+VTC_INDEX_CODE_%s\s+%d\b' % (name, value),
                     code), name
  assert (data.ABSENT, data.MAX_COLUMNS, data.MAX_SYMBOLS) == (255, 4096, 4096)
  assert '#include "vtc_quality.h"' in code


def test_the_nine_headers_do_not_overlap():
  for other in OTHER_HEADERS:
    names = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(other)))
    assert names and not names & set(declarations()), other.name


def test_binding_table_is_the_declared_surface():
  vtc_hip, lib = _lib()
  assert sorted(vtc_hip.INDEX_CODE_SIGNATURES) == sorted(declarations())
  for other in (vtc_hip.SIGNATURES, vtc_hip.IMAGE_SIGNATURES,
                vtc_hip.CODEC_SIGNATURES, vtc_hip.DECODE_SIGNATURES,
                vtc_hip.QUALITY_SIGNATURES, vtc_hip.STATS_SIGNATURES,
                vtc_hip.QUANT_SIGNATURES, vtc_hip.VQ_SIGNATURES):
    assert not set(vtc_hip.INDEX_CODE_SIGNATURES) & set(other)
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declarations().items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.INDEX_CODE_SIGNATURES[name][1]) == count, name
    assert getattr(lib, name).argtypes == (
        vtc_hip.INDEX_CODE_SIGNATURES[name][1])
  assert (lib.vtc_index_code_abi_version() ==
          vtc_hip.INDEX_CODE_ABI_VERSION == 1)
  assert (vtc_hip.INDEX_CODE_ABSENT, vtc_hip.INDEX_CODE_MAX_COLUMNS,
          vtc_hip.INDEX_CODE_MAX_SYMBOLS) == (data.ABSENT, data.MAX_COLUMNS,
                                              data.MAX_SYMBOLS)
  # the other eight stay where they were
  assert (lib.vtc_abi_version(), lib.vtc_image_abi_version(),
          lib.vtc_codec_abi_version(), lib.vtc_decode_abi_version(),
          lib.vtc_quality_abi_version(), lib.vtc_stats_abi_version(),
          lib.vtc_quant_abi_version(), lib.vtc_vq_abi_version()) == (
              4, 1, 1, 1, 1, 1, 1, 1)
  assert len(vtc_hip.QUANT_SIGNATURES) == 5
  assert len(vtc_hip.VQ_SIGNATURES) == 5
  assert len(vtc_hip.CODEC_SIGNATURES) == 8


def _refused(lib, rc, status, *words):
  assert rc == status, (rc, lib.vtc_last_error())
  text = lib.vtc_last_error().decode()
  for word in words:
    assert word in text, text


def test_argument_errors_do_not_touch_the_gpu():
  """Null pointers, bad sizes and unsupported sizes, one argument at a time.
  The non-null pointers are host integers that are never dereferenced: this
  runs with no device."""
  _, lib = _lib()
  p = [ctypes.c_void_p(v << 20) for v in range(1, 12)]

  who = 'vtc_index_code_bits'
  #       indices b   m   len  kmax rows  cols  status stream
  good = [p[0], 257, 42, p[1], 40, p[2], p[3], p[4], None]
  for position in (0, 3, 5, 6, 7):
    args = list(good)
    args[position] = None
    _refused(lib, lib.vtc_index_code_bits(*args), ERR_INVALID_ARGUMENT, who,
             'null')
  for position, value, word in ((1, 0, 'b = 0'), (1, -3, 'b = -3'),
                                (2, 0, 'm = 0'), (2, -1, 'm = -1'),
                                (4, 0, 'kmax = 0')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_index_code_bits(*args), ERR_INVALID_ARGUMENT, who,
             word)
  for position, value, word in ((2, 4097, 'm = 4097'),
                                (4, 4097, 'kmax = 4097'),
                                (1, 1 << 44, 'too many rows')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_index_code_bits(*args), ERR_UNSUPPORTED, who, word)

  who = 'vtc_index_code_pack'
  #       indices b   m  code  len  kmax offsets packed bytes status stream
  good = [p[0], 257, 42, p[1], p[2], 40, p[3], p[4], 1000, p[5], None]
  for position in (0, 3, 4, 6, 7, 9):
    args = list(good)
    args[position] = None
    _refused(lib, lib.vtc_index_code_pack(*args), ERR_INVALID_ARGUMENT, who,
             'null')
  for position, value, word in ((1, 0, 'b = 0'), (2, 0, 'm = 0'),
                                (5, 0, 'kmax = 0'), (5, -7, 'kmax = -7'),
                                (8, -1, 'packed_bytes = -1'),
                                (8, 1 << 59, 'packed_bytes')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_index_code_pack(*args), ERR_INVALID_ARGUMENT, who,
             word)
  for position, value, word in ((2, 4097, 'm = 4097'),
                                (5, 4097, 'kmax = 4097')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_index_code_pack(*args), ERR_UNSUPPORTED, who, word)


def test_cpu_tensors_are_refused():
  import torch
  import vtc_hip
  from utils import index_coding
  indices = torch.zeros((4, 2), dtype=torch.int32)
  tables = [{0: '0', 1: '1'}, {0: ''}]
  with pytest.raises(vtc_hip.VtcHipError):
    index_coding.index_code_bits(indices, tables)
  with pytest.raises(vtc_hip.VtcHipError):
    index_coding.pack_index_streams(indices, tables)


# ------------------------------------------------------------ Huffman tables
def _properties(table, weights):
  from utils import jpeg
  assert sorted(table) == list(range(len(weights)))
  assert all(set(word) <= {'0', '1'} for word in table.values())
  jpeg.check_prefix_free(table) if len(table) > 1 else None
  if len(table) >= 2:
    numerator, longest = data.kraft_numerator(table)
    assert numerator == 1 << longest          # Kraft's sum is exactly 1
  assert data.table_cost(table, weights) == data.huffman_cost(weights)


@pytest.mark.parametrize('seed,kmax,k', [(1, 16, 16), (2, 64, 40),
                                         (3, 300, 300), (4, 4096, 4096),
                                         (5, 4096, 1000)])
def test_tables_are_optimal_prefix_codes(seed, kmax, k):
  from utils import index_coding
  rs = np.random.RandomState(seed)
  counts = np.stack([data.geometric_counts(seed, kmax, k),
                     rs.randint(0, 50, size=kmax) * (np.arange(kmax) < k),
                     np.zeros(kmax, np.int64)])          # nothing seen at all
  tables = index_coding.index_huffman_tables(counts, k)
  assert len(tables) == 3
  for j, table in enumerate(tables):
    weights = data.training_weights(counts[j], k)
    assert len(weights) == k and min(weights) >= 1
    _properties(table, weights)
    # unseen i < k are present, i >= k absent
    assert all(i in table for i in range(k) if counts[j, i] == 0)
    assert not any(i in table for i in range(k, kmax))
  # seen indices keep their counts: a heavier symbol never has a longer word
  weights = data.training_weights(counts[0], k)
  spans = {}
  for i, w in enumerate(weights):
    lo, hi = spans.get(w, (99, 0))
    spans[w] = (min(lo, len(tables[0][i])), max(hi, len(tables[0][i])))
  ordered = [spans[w] for w in sorted(spans, reverse=True)]
  assert all(a[1] <= b[0] for a, b in zip(ordered, ordered[1:]))
  # deterministic
  assert tables == index_coding.index_huffman_tables(counts.tolist(), [k] * 3)


def test_k_per_column_and_one_symbol_columns():
  from utils import index_coding
  counts = np.array([[5, 0, 0, 9], [0, 0, 0, 0], [3, 1, 0, 0]])
  tables = index_coding.index_huffman_tables(counts, [4, 1, 3])
  assert tables[1] == {0: ''}
  assert sorted(tables[0]) == [0, 1, 2, 3] and sorted(tables[2]) == [0, 1, 2]
  assert len(tables[0][3]) == 1 and len(tables[0][0]) == 2
  assert {len(tables[0][1]), len(tables[0][2])} == {3}
  for j, k in enumerate([4, 1, 3]):
    _properties(tables[j], data.training_weights(counts[j], k))
  # a [kmax] row is one column (vector_index_counts)
  assert index_coding.index_huffman_tables(counts[0]) == [tables[0]]
  for bad in ([4, 1], [4, 0, 3], [5, 1, 3]):
    with pytest.raises(ValueError):
      index_coding.index_huffman_tables(counts, bad)
  code, length = index_coding.index_table_arrays(tables, 4)
  assert code.dtype == np.uint64 and length.dtype == np.uint8
  assert length[1].tolist() == [0, 255, 255, 255]
  assert length[2].tolist()[3] == 255 and code[1].tolist() == [0, 0, 0, 0]
  for j, table in enumerate(tables):
    for i, word in table.items():
      assert length[j, i] == len(word)
      assert int(code[j, i]) == (int(word, 2) if word else 0)


def test_codewords_of_1_to_64_bits_and_one_more():
  from utils import index_coding
  weights = data.long_weights()
  assert len(weights) == 65 and weights[-1] == 1 << 64
  table = index_coding.index_huffman_tables([weights])[0]
  lengths = [len(table[i]) for i in range(65)]
  assert lengths == [64] + list(range(64, 0, -1))
  _properties(table, weights)
  code, length = index_coding.index_table_arrays([table], 70)
  assert length[0, :65].tolist() == lengths
  assert (length[0, 65:] == 255).all()
  for i in range(65):
    assert format(int(code[0, i]), 'b').zfill(lengths[i]) == table[i]
  # the tests on the device use its complement, which sets the high bits
  flipped = data.complement(table)
  _properties(flipped, weights)
  assert [len(flipped[i]) for i in range(65)] == lengths
  code, _ = index_coding.index_table_arrays([flipped], 65)
  assert int(code[0].max()) == (1 << 64) - 1
  longer = index_coding.index_huffman_tables([data.long_weights(66)])
  assert max(len(word) for word in longer[0].values()) == 65
  with pytest.raises(NotImplementedError):
    index_coding.index_table_arrays(longer, 66)


# -------------------------------------------------------------- restatement
def test_restatement_on_a_hand_worked_case():
  tables = [{0: '0', 1: '10', 2: '11'}, {0: ''}, {0: '1', 3: '0'}]
  indices = np.array([[1, 0, 3], [0, 0, 0], [2, 0, 1], [-1, 0, 3]], np.int32)
  assert data.row_bits(indices, tables).tolist() == [3, 2, 2, 1]
  assert data.column_bits(indices, tables).tolist() == [5, 0, 3]
  assert [data.stream(row, tables) for row in indices] == ['100', '01', '11',
                                                           '0']
  assert data.status(indices, tables) == [2, 1 + 2 * 3 + 2]
  assert data.status(indices[:2], tables) == [0, 0]
  offsets = data.layout([3, 2, 2, 1], 3, [0, 5, 1, 0])
  assert offsets.tolist() == [3, 6, 13, 16, 17]
  got, dropped = data.image(indices, tables, offsets, 3)
  #              ...100 01..... 11 0
  assert ''.join('%d' % v for v in np.unpackbits(got)) == (
      '000100010000011000000000') and dropped == 0
  got, dropped = data.image(indices, tables, offsets, 1)
  assert got.tolist() == [0b00010001] and dropped == 3
  # a row cut by the next offset, a decreasing and a negative offset
  got, dropped = data.image(indices, tables, np.array([0, 2, 2, 1, 4]), 1)
  assert dropped == 1 + 2 + 2 and got.tolist() == [0b10000000]
  got, dropped = data.image(indices[:1], tables, np.array([-1, 5]), 1)
  assert dropped == 3 and got.tolist() == [0]
  assert data.huffman_cost([1, 1, 2, 4]) == 2 + 4 + 8
  assert data.huffman_cost([5]) == 0
  assert abs(data.entropy_bits(np.array([[0], [0], [1], [2]]), 3) - 6.0) < 1e-12


def test_shared_cases_cover_what_they_claim():
  """The tables and indices the GPU tests share: lengths from 1 to about 18
  in the trained columns, the 32-, 33- and 64-bit codewords in use, a
  one-symbol column and a column with k < kmax wherever there is room."""
  assert len(data.SHAPES) == 12
  for b, m, kmax in data.SHAPES:
    tables, k = data.case_tables(b, m, kmax)
    indices = data.case_indices(b, m, kmax)
    kinds = data.column_kinds(b, m, kmax)
    assert indices.shape == (b, m) and len(tables) == m
    assert data.status(indices, tables) == [0, 0]
    for j, kind in enumerate(kinds):
      used = {len(tables[j][int(i)]) for i in indices[:, j]}
      if kind == 'long' and b >= 3:
        assert {32, 33, 64} <= used
      if kind == 'one':
        assert tables[j] == {0: ''}
      if kind == 'short':
        assert k[j] < kmax and kmax - 1 not in tables[j]
    if m > 1:
      assert 'one' in kinds and 'short' in kinds
  lengths = {len(w) for w in data.case_tables(257, 1, 4096)[0][0].values()}
  assert min(lengths) == 1 and 17 <= max(lengths) <= 22
  assert data.row_bits(data.case_indices(2, 4096, 4),
                       data.case_tables(2, 4096, 4)[0]).max() > 4096
