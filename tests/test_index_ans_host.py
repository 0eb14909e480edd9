"""The eleventh header, include/vtc_index_ans.h, held to what
tests/test_index_decode_host.py asks of the tenth: INDEX_ANS_SIGNATURES is
exactly the declared surface and shares no name with the other ten tables; the
library exports it; bad arguments are answered before any device work; the
workspace query is host-only.  Then the restatement of
tests/index_ans_data.py: it reads back what it writes for every shared case,
the frequency rule against the product's, and the two rate conditions of the
sparse scene.  No GPU needed."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import index_ans_data as truth
import index_code_data as huffman

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'vtc_index_ans.h'
OTHER_HEADERS = [REPO / 'include' / name
                 for name in ('vtc_hip.h', 'vtc_image.h', 'vtc_codec.h',
                              'vtc_decode.h', 'vtc_quality.h', 'vtc_stats.h',
                              'vtc_quant.h', 'vtc_vq.h', 'vtc_index_code.h',
                              'vtc_index_decode.h')]

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
      'vtc_index_ans_abi_version', 'vtc_index_ans_pack', 'vtc_index_ans_sizes',
      'vtc_index_ans_unpack', 'vtc_index_ans_workspace_bytes']
  code = _code(HEADER)
  assert re.search(r'#define\s+VTC_INDEX_ANS_ABI_VERSION\s+1\b', code)
  assert re.search(r'#define\s+VTC_INDEX_ANS_PROB_BITS\s+%d\b'
                   % truth.PROB_BITS, code)
  assert re.search(r'#define\s+VTC_INDEX_ANS_LANES\s+%d\b' % truth.LANES, code)
  assert '#include "vtc_index_decode.h"' in code


def test_the_eleven_headers_do_not_overlap():
  for other in OTHER_HEADERS:
    names = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(other)))
    assert names and not names & set(declarations()), other.name


def test_binding_table_is_the_declared_surface():
  vtc_hip, lib = _lib()
  assert sorted(vtc_hip.INDEX_ANS_SIGNATURES) == sorted(declarations())
  for other in (vtc_hip.SIGNATURES, vtc_hip.IMAGE_SIGNATURES,
                vtc_hip.CODEC_SIGNATURES, vtc_hip.DECODE_SIGNATURES,
                vtc_hip.QUALITY_SIGNATURES, vtc_hip.STATS_SIGNATURES,
                vtc_hip.QUANT_SIGNATURES, vtc_hip.VQ_SIGNATURES,
                vtc_hip.INDEX_CODE_SIGNATURES,
                vtc_hip.INDEX_DECODE_SIGNATURES):
    assert not set(vtc_hip.INDEX_ANS_SIGNATURES) & set(other)
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declarations().items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.INDEX_ANS_SIGNATURES[name][1]) == count, name
    assert getattr(lib, name).argtypes == vtc_hip.INDEX_ANS_SIGNATURES[name][1]
  assert (lib.vtc_index_ans_abi_version() ==
          vtc_hip.INDEX_ANS_ABI_VERSION == 1)
  assert vtc_hip.INDEX_ANS_PROB_BITS == truth.PROB_BITS
  assert vtc_hip.INDEX_ANS_LANES == truth.LANES
  assert 1 << vtc_hip.INDEX_ANS_MAX_STREAM_BITS == truth.MAX_STREAM_SYMBOLS
  # the other ten stay where they were
  assert (lib.vtc_abi_version(), lib.vtc_image_abi_version(),
          lib.vtc_codec_abi_version(), lib.vtc_decode_abi_version(),
          lib.vtc_quality_abi_version(), lib.vtc_stats_abi_version(),
          lib.vtc_quant_abi_version(), lib.vtc_vq_abi_version(),
          lib.vtc_index_code_abi_version(),
          lib.vtc_index_decode_abi_version()) == (4, 1, 1, 1, 1, 1, 1, 1, 1, 1)
  assert len(vtc_hip.INDEX_CODE_SIGNATURES) == 3
  assert len(vtc_hip.INDEX_DECODE_SIGNATURES) == 3


def _refused(lib, rc, status, *words):
  assert rc == status, (rc, lib.vtc_last_error())
  text = lib.vtc_last_error().decode()
  for word in words:
    assert word in text, text


def _good_calls(lib):
  """name -> (function, good arguments, positions of the pointers that must
  not be null, positions of b, m, kmax, rows, packed_bytes or None, of the
  workspace pointer).  The non-null pointers are host integers that are never
  dereferenced."""
  p = [ctypes.c_void_p(v << 20) for v in range(1, 12)]
  need = lib.vtc_index_ans_workspace_bytes(42, 40)
  assert need > 0
  return need, {
      #                      indices b   m   freq kmax R  sizes status ws
      'vtc_index_ans_sizes': (
          lib.vtc_index_ans_sizes,
          [p[0], 257, 42, p[1], 40, 100, p[2], p[3], p[4], need, None],
          (0, 3, 6, 7), (1, 2, 4, 5, None), 8),
      #                     indices b   m   freq kmax R  sizes offsets packed
      'vtc_index_ans_pack': (
          lib.vtc_index_ans_pack,
          [p[0], 257, 42, p[1], 40, 100, p[2], p[3], p[4], 1000, p[5], p[6],
           need, None],
          (0, 3, 6, 7, 8, 10), (1, 2, 4, 5, 9), 11),
      #                       packed bytes offsets b  m   freq kmax R
      'vtc_index_ans_unpack': (
          lib.vtc_index_ans_unpack,
          [p[0], 1000, p[1], 257, 42, p[2], 40, 100, p[3], p[4], p[5], p[6],
           need, None],
          (0, 2, 5, 8, 9, 10), (3, 4, 6, 7, 1), 11)}


def test_argument_errors_do_not_touch_the_gpu():
  """Null pointers, bad sizes, unsupported sizes and a short workspace, one
  argument at a time, for the three calls.  This runs with no device."""
  _, lib = _lib()
  need, calls = _good_calls(lib)
  for who, (fn, good, pointers, sizes, ws_at) in calls.items():
    at_b, at_m, at_kmax, at_rows, at_bytes = sizes
    for position in pointers:
      args = list(good)
      args[position] = None
      _refused(lib, fn(*args), ERR_INVALID_ARGUMENT, who, 'null')
    bad = [(at_b, 0, 'b = 0'), (at_b, -3, 'b = -3'), (at_m, 0, 'm = 0'),
           (at_m, -1, 'm = -1'), (at_kmax, 0, 'kmax = 0'),
           (at_kmax, -7, 'kmax = -7'), (at_rows, 0, 'rows_per_stream = 0'),
           (at_rows, -2, 'rows_per_stream = -2')]
    if at_bytes is not None:
      bad += [(at_bytes, -1, 'packed_bytes = -1'),
              (at_bytes, 1 << 59, 'packed_bytes')]
    for position, value, word in bad:
      args = list(good)
      args[position] = value
      _refused(lib, fn(*args), ERR_INVALID_ARGUMENT, who, word)
    for position, value, word in ((at_m, 4097, 'm = 4097'),
                                  (at_kmax, 4097, 'kmax = 4097'),
                                  (at_rows, (1 << 24) // 42 + 1,
                                   'rows_per_stream * m')):
      args = list(good)
      args[position] = value
      _refused(lib, fn(*args), ERR_UNSUPPORTED, who, word)
    # R * m = 2^24 exactly is taken (answered by the short workspace below)
    args = list(good)
    args[at_m], args[at_rows], args[ws_at + 1] = 4096, 4096, 0
    _refused(lib, fn(*args), ERR_WORKSPACE, who, 'workspace')
    # too many streams for one grid
    args = list(good)
    args[at_b], args[at_rows] = 1 << 44, 1
    _refused(lib, fn(*args), ERR_UNSUPPORTED, who, 'too many streams')
    # the workspace: null, one byte short, none
    for pointer, nbytes in ((None, need), (good[ws_at], need - 1),
                            (good[ws_at], 0)):
      args = list(good)
      args[ws_at], args[ws_at + 1] = pointer, nbytes
      _refused(lib, fn(*args), ERR_WORKSPACE, who, 'workspace',
               '%d needed' % need)


def test_workspace_query():
  """Host-only (no device here), monotone in m and kmax, the documented sum,
  0 for the sizes the calls refuse."""
  _, lib = _lib()
  query = lib.vtc_index_ans_workspace_bytes

  def up(v):
    return -(-v // 256) * 256

  for m, kmax in ((1, 1), (1, 4096), (42, 1024), (5, 300), (4096, 4),
                  (4096, 4096)):
    assert query(m, kmax) == (up(2 * m * kmax) + up(2 * 256 * m) +
                              up(4)), (m, kmax)
  sizes = (1, 2, 63, 64, 65, 300, 1024, 4095, 4096)
  for a, b in zip(sizes, sizes[1:]):
    assert query(a, 40) <= query(b, 40) and query(42, a) <= query(42, b)
    assert query(a, a) <= query(b, b)
  for m, kmax in ((0, 40), (-1, 40), (4097, 40), (42, 0), (42, -5),
                  (42, 4097)):
    assert query(m, kmax) == 0, (m, kmax)


def test_cpu_tensors_and_bad_arguments_are_refused():
  import torch
  import vtc_hip
  from utils import index_coding
  from utils import quantization
  freq = truth.frequency_array([[5, 1, 0, 9], [1, 1, 1, 1]])
  indices = torch.zeros((3, 2), dtype=torch.int32)
  packed = torch.zeros(512, dtype=torch.uint8)
  offsets = torch.zeros(2, dtype=torch.int64)
  with pytest.raises(vtc_hip.VtcHipError):
    index_coding.index_ans_stream_bytes(indices, freq)
  with pytest.raises(vtc_hip.VtcHipError):
    index_coding.pack_index_ans(indices, freq)
  with pytest.raises(vtc_hip.VtcHipError):
    index_coding.unpack_index_ans(packed, offsets, freq, 3, 3)
  with pytest.raises(vtc_hip.VtcHipError):
    quantization.decode_codes(packed, offsets, freq, np.zeros((2, 4)),
                              ans_shape=(3, 3))
  with pytest.raises(ValueError):
    index_coding.index_ans_frequencies([[1, 2, 3]], k=4)
  with pytest.raises(ValueError):
    index_coding.index_ans_frequencies([[1, -2, 3]])


# -------------------------------------------------------------- frequencies
def _check_frequencies(freq, counts, k):
  assert freq.dtype == np.uint16 and freq.shape == np.asarray(counts).shape
  for row, kj in zip(freq, k):
    assert int(row.astype(np.int64).sum()) == truth.SCALE
    assert (row[:kj] >= 1).all() and (row[kj:] == 0).all()


def test_frequencies_follow_the_rule():
  from utils import index_coding
  rs = np.random.RandomState(3)
  cases = [
      ([[7]], [1]),                                  # k = 1: 2^15
      ([[7, 0, 0, 0]], [1]),
      ([[0] * 4096], [4096]),                        # every count 0: 8 each
      ([[5] * 4096], [4096]),                        # all equal
      ([[10 ** 9] + [0] * 299], [300]),              # one dominant count
      ([[10 ** 12, 3, 1, 0, 0, 2]], [5]),
      ([[3, 3, 3]], [3]),                            # 2^15 is no multiple of 3
      (rs.randint(0, 50, size=(6, 300)).tolist(), [300, 299, 150, 2, 1, 64]),
      ([truth._geometric_counts(5, 4096, 4096).tolist()], [4096]),
  ]
  for counts, k in cases:
    got = index_coding.index_ans_frequencies(counts, k)
    _check_frequencies(got, counts, k)
    assert np.array_equal(got, truth.frequency_array(counts, k))
  assert index_coding.index_ans_frequencies([[7]]).tolist() == [[truth.SCALE]]
  assert index_coding.index_ans_frequencies([[0] * 4096]).tolist() == [
      [8] * 4096]
  assert index_coding.index_ans_frequencies([[5] * 4096]).tolist() == [
      [8] * 4096]
  dominant = index_coding.index_ans_frequencies([[10 ** 9] + [0] * 4095])[0]
  assert dominant.tolist() == [truth.SCALE - 4095] + [1] * 4095
  # the remainder goes to the heaviest first, ties by index
  assert index_coding.index_ans_frequencies([[3, 3, 3]]).tolist() == [
      [10923, 10923, 10922]]
  assert index_coding.index_ans_frequencies([[1, 2, 1]], k=3).tolist() == [
      [8192, 16384, 8192]]
  # one k for all columns, a 1-d row of counts
  got = index_coding.index_ans_frequencies(np.array([4, 0, 4]), k=2)
  assert np.array_equal(got, np.array([[26215, 6553, 0]], np.uint16))


# -------------------------------------------------------------- restatement
def test_restatement_on_a_hand_worked_case():
  """Two symbols of frequency 2^14 each are one bit each: 64 x 17 of them
  leave 64 states and 64 words."""
  freq = np.array([[1 << 14, 1 << 14]], np.uint16)
  indices = np.zeros((64 * 17, 1), np.int32)
  streams, status = truth.encode(indices, freq, 64 * 17)
  assert status == [0, 0, 0] and len(streams) == 1
  # a lane starts at 2^16 and gains one bit per symbol: after 16 symbols it is
  # 2^32 / ... it emits exactly one word on the way to 17 symbols
  assert len(streams[0]) == truth.HEADER + 2 * 64
  # a one-symbol column costs nothing and leaves the states at L
  one = np.array([[truth.SCALE, 0, 0]], np.uint16)
  streams, status = truth.encode(np.zeros((1000, 1), np.int32), one, 1000)
  assert streams == [(truth.LOWER).to_bytes(4, 'little') * 64]
  # an absent symbol 0 and one between present ones are skipped by the search
  gap = np.array([[0, 100, 0, truth.SCALE - 100, 0]], np.uint16)
  host = np.array([[1], [3], [3], [1]], np.int32)
  streams, status = truth.encode(host, gap, 4)
  packed = np.frombuffer(streams[0], np.uint8)
  got, used, status = truth.decode(packed, [0, len(packed)], 4, 1, gap, 4)
  assert np.array_equal(got, host) and status == [0, 0, 0]
  assert used.tolist() == [len(packed)]
  # uncodable entries: negative, >= kmax, frequency 0
  host = np.array([[1], [0], [-1], [5], [3], [2]], np.int32)
  streams, status = truth.encode(host, gap, 4)
  assert status == [4, 2, 0] and len(streams) == 2
  # a bad column codes nothing
  bad = np.array([[1, 2], [truth.SCALE, 0], [3, 4]], np.uint16)
  streams, status = truth.encode(np.zeros((5, 3), np.int32), bad, 2)
  assert streams == [b''] * 3 and status == [0, 0, 1]
  got, used, status = truth.decode(np.zeros(9, np.uint8), [0, 3, 6, 9], 5, 3,
                                   bad, 2)
  assert (got == -1).all() and (used == 0).all() and status == [0, 0, 1]


@pytest.mark.parametrize('case', truth.CASES, ids=truth.IDS)
def test_restatement_round_trips_every_case(case):
  b, m, kmax, rows = case
  freq, host = truth.case_freq(*case), truth.case_indices(*case)
  streams = truth.case_streams(*case)
  n = truth.streams_of(b, rows)
  assert len(streams) == n
  assert all(len(s) >= truth.HEADER and len(s) % 2 == 0 for s in streams)
  sizes = [len(s) for s in streams]
  for lead in (0, 3):
    offsets = truth.layout(sizes, lead, truth.gaps(n))
    packed, skipped = truth.image(streams, offsets, int(offsets[-1]))
    assert skipped == 0
    got, used, status = truth.decode(packed, offsets, b, m, freq, rows)
    assert status == [0, 0, 0]
    assert np.array_equal(got, host) and used.tolist() == sizes
  # the bytes are at least the ideal cost of the frequencies, and every
  # stream's excess is below its flush of 64 states of 32 bits
  ideal = truth.ideal_bits(host, freq)
  assert 8 * sum(sizes) >= ideal
  assert 8 * sum(sizes) <= ideal + n * (8 * truth.HEADER + 16) + 0.01 * ideal


def test_restatement_classifies_damaged_streams():
  case = (257, 42, 64, 100)
  b, m, kmax, rows = case
  freq = truth.case_freq(*case)
  host = truth.case_indices(*case)
  streams, _ = truth.encode(host, freq, rows)
  sizes = [len(s) for s in streams]
  offsets = truth.layout(sizes, 0, [0, 0, 0])
  packed, _ = truth.image(streams, offsets, int(offsets[-1]))
  # the middle slot cut by two bytes: it runs dry in its last steps
  cut = offsets.copy()
  cut[2] -= 2
  shifted = np.concatenate([packed[:cut[2]], packed[offsets[2]:]])
  moved = np.array([cut[0], cut[1], cut[2], cut[3] - 2])
  got, used, status = truth.decode(shifted, moved, b, m, freq, rows)
  assert status == [1, 2, 0]
  assert np.array_equal(got[:100], host[:100])
  assert np.array_equal(got[200:], host[200:])
  middle = got[100:200].reshape(-1)
  dry = np.nonzero(middle < 0)[0]
  assert len(dry) and dry[0] % 64 == 0 and (middle[dry[0]:] == -1).all()
  assert np.array_equal(middle[:dry[0]], host[100:200].reshape(-1)[:dry[0]])
  # one flipped word: everything decodes to something, the end states tell
  flipped = packed.copy()
  flipped[offsets[1] + truth.HEADER + 10] ^= 0x40
  got, used, status = truth.decode(flipped, offsets, b, m, freq, rows)
  assert status[:2] == [1, 2]
  assert np.array_equal(got[:100], host[:100])
  assert np.array_equal(got[200:], host[200:])
  # offsets that decrease; a negative one
  wrong = offsets.copy()
  wrong[1] = offsets[2] + 4
  got, used, status = truth.decode(packed, wrong, b, m, freq, rows)
  assert status[1] in (1, 2) and (got[100:200] == -1).all()
  assert used[1] == 0


# -------------------------------------------------------------------- rates
def test_rate_conditions_on_the_restatement():
  """The sparse scene: the range coder's bytes are strictly below the Huffman
  bits of the same indices, and not below their in-sample entropy."""
  from utils import index_coding
  b, m, kmax, rows = truth.RATE_SCENE
  host = truth.sparse_indices(11, b, m, kmax)
  assert 0.88 < float((host == 0).mean()) < 0.92
  counts = np.stack([np.bincount(host[:, j], minlength=kmax)
                     for j in range(m)])
  freq = truth.frequency_array(counts)
  tables = index_coding.index_huffman_tables(counts)
  huffman_bits = int(huffman.row_bits(host, tables).sum())
  ans_bits = 8 * truth.total_bytes(host, freq, rows)
  entropy = truth.entropy_bits(host, kmax)
  ideal = truth.ideal_bits(host, freq)
  print('index_ans_rate per index: entropy %.4f ideal %.4f ans %.4f '
        'huffman %.4f' % tuple(v / float(b * m) for v in
                               (entropy, ideal, ans_bits, huffman_bits)))
  assert ans_bits < huffman_bits
  assert ans_bits >= entropy
  assert ideal >= entropy and ans_bits >= ideal
