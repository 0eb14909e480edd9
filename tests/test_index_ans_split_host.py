"""The thirteenth header, include/ext/vtc_index_ans_split.h, held to what
tests/test_index_ans_host.py asks of the eleventh: INDEX_ANS_SPLIT_BINDINGS
is exactly the declared surface and shares no name with the other tables; the
library exports it; bad arguments are answered before any device work; the
workspace query is host-only.  Then the restatement of
tests/index_ans_split_data.py: the frequency rule against hand-worked values
and the product's, round trips of every shared case, the cost bound on three
sparse scenes, damaged streams.  No GPU needed."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import index_ans_split_data as truth

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'ext' / 'vtc_index_ans_split.h'
OTHER_HEADERS = sorted((REPO / 'include').glob('*.h'))

OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, 1, 2, 3
ENTRY_POINTS = ['vtc_index_ans_split_abi_version', 'vtc_index_ans_split_pack',
                'vtc_index_ans_split_sizes', 'vtc_index_ans_split_unpack',
                'vtc_index_ans_split_workspace_bytes']
SCALE, LO = truth.SCALE, truth.LO


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
  assert sorted(declarations()) == ENTRY_POINTS
  code = _code(HEADER)
  assert re.search(r'#define\s+VTC_INDEX_ANS_SPLIT_ABI_VERSION\s+1\b', code)
  assert re.search(r'#define\s+VTC_INDEX_ANS_SPLIT_MAX_SYMBOLS\s+%d\b'
                   % truth.MAX_SYMBOLS, code)
  assert re.search(r'#define\s+VTC_INDEX_ANS_SPLIT_LO_BITS\s+%d\b'
                   % truth.LO_BITS, code)
  assert truth.MAX_SYMBOLS == 131072 and truth.LO_BITS == 8
  assert '#include "../vtc_index_ans.h"' in code
  # the eleventh header's constants are reused, not restated
  assert 'PROB_BITS' not in code and 'LANES' not in code
  assert 'asm' not in code


def test_the_headers_do_not_overlap():
  assert len(OTHER_HEADERS) >= 12 and HEADER not in OTHER_HEADERS
  for other in OTHER_HEADERS:
    names = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(other)))
    assert names and not names & set(declarations()), other.name
  makefile = (REPO / 'vision-transform-codes_amd' / 'csrc' /
              'Makefile').read_text()
  assert 'include/ext/vtc_index_ans_split.h' in makefile


def test_binding_table_is_the_declared_surface():
  vtc_hip, lib = _lib()
  assert sorted(vtc_hip.INDEX_ANS_SPLIT_BINDINGS) == ENTRY_POINTS
  tables = [getattr(vtc_hip, name) for name in dir(vtc_hip)
            if name.endswith('SIGNATURES')]
  assert len(tables) >= 12
  for other in tables:
    assert not set(vtc_hip.INDEX_ANS_SPLIT_BINDINGS) & set(other)
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declarations().items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.INDEX_ANS_SPLIT_BINDINGS[name][1]) == count, name
    assert (getattr(lib, name).argtypes ==
            vtc_hip.INDEX_ANS_SPLIT_BINDINGS[name][1])
  assert (lib.vtc_index_ans_split_abi_version() ==
          vtc_hip.INDEX_ANS_SPLIT_ABI_VERSION == 1)
  assert vtc_hip.INDEX_ANS_SPLIT_MAX_SYMBOLS == truth.MAX_SYMBOLS
  assert vtc_hip.INDEX_ANS_SPLIT_LO_BITS == truth.LO_BITS
  # the first and the eleventh header stay where they were
  assert lib.vtc_abi_version() == vtc_hip.ABI_VERSION == 4
  assert lib.vtc_index_ans_abi_version() == vtc_hip.INDEX_ANS_ABI_VERSION == 1
  assert len(vtc_hip.INDEX_ANS_SIGNATURES) == 5


def _refused(lib, rc, status, *words):
  assert rc == status, (rc, lib.vtc_last_error())
  text = lib.vtc_last_error().decode()
  for word in words:
    assert word in text, text


KMAX = 5000


def _good_calls(lib):
  """name -> (function, good arguments, positions of the pointers that must
  not be null, positions of b, kmax, rows, packed_bytes or None, of the
  workspace pointer).  The non-null pointers are host integers that are never
  dereferenced."""
  p = [ctypes.c_void_p(v << 20) for v in range(1, 12)]
  need = lib.vtc_index_ans_split_workspace_bytes(KMAX)
  assert need > 0
  return need, {
      #        indices b  freq_hi freq_lo kmax R  sizes status ws
      'vtc_index_ans_split_sizes': (
          lib.vtc_index_ans_split_sizes,
          [p[0], 300, p[1], p[2], KMAX, 100, p[3], p[4], p[5], need, None],
          (0, 2, 3, 6, 7), (1, 4, 5, None), 8),
      #        indices b  freq_hi freq_lo kmax R  sizes offsets packed bytes
      'vtc_index_ans_split_pack': (
          lib.vtc_index_ans_split_pack,
          [p[0], 300, p[1], p[2], KMAX, 100, p[3], p[4], p[5], 1000, p[6],
           p[7], need, None],
          (0, 2, 3, 6, 7, 8, 10), (1, 4, 5, 9), 11),
      #        packed bytes offsets b freq_hi freq_lo kmax R indices used
      'vtc_index_ans_split_unpack': (
          lib.vtc_index_ans_split_unpack,
          [p[0], 1000, p[1], 300, p[2], p[3], KMAX, 100, p[4], p[5], p[6],
           p[7], need, None],
          (0, 2, 4, 5, 8, 9, 10), (3, 6, 7, 1), 11)}


def test_argument_errors_do_not_touch_the_gpu():
  """Null pointers, bad sizes, unsupported sizes and a short workspace, one
  argument at a time, for the three calls.  This runs with no device."""
  _, lib = _lib()
  need, calls = _good_calls(lib)
  for who, (fn, good, pointers, sizes, ws_at) in calls.items():
    at_b, at_kmax, at_rows, at_bytes = sizes
    for position in pointers:
      args = list(good)
      args[position] = None
      _refused(lib, fn(*args), ERR_INVALID_ARGUMENT, who, 'null')
    bad = [(at_b, 0, 'b = 0'), (at_b, -3, 'b = -3'),
           (at_kmax, 0, 'kmax = 0'), (at_kmax, -7, 'kmax = -7'),
           (at_rows, 0, 'rows_per_stream = 0'),
           (at_rows, -2, 'rows_per_stream = -2')]
    if at_bytes is not None:
      bad += [(at_bytes, -1, 'packed_bytes = -1'),
              (at_bytes, 1 << 59, 'packed_bytes')]
    for position, value, word in bad:
      args = list(good)
      args[position] = value
      _refused(lib, fn(*args), ERR_INVALID_ARGUMENT, who, word)
    for position, value, word in ((at_kmax, 131073, 'kmax = 131073'),
                                  (at_rows, (1 << 24) + 1,
                                   'rows_per_stream = 16777217')):
      args = list(good)
      args[position] = value
      _refused(lib, fn(*args), ERR_UNSUPPORTED, who, word)
    # kmax = 131072 and R = 2^24 exactly are taken (answered by the short
    # workspace below)
    args = list(good)
    args[at_kmax], args[at_rows], args[ws_at + 1] = 131072, 1 << 24, 0
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
  """Host-only (no device here), monotone in kmax, the documented sum, 0 for
  the sizes the calls refuse."""
  _, lib = _lib()
  query = lib.vtc_index_ans_split_workspace_bytes

  def up(v):
    return -(-v // 256) * 256

  sizes = (1, 2, 255, 256, 257, 4096, 4097, 5000, 65536, 131071, 131072)
  for kmax in sizes:
    top = truth.hi_symbols(kmax)
    assert query(kmax) == up(2 * top) + up(2 * top * LO) + up(4), kmax
  for a, b in zip(sizes, sizes[1:]):
    assert query(a) <= query(b)
  assert query(131072) == 1024 + 262144 + 256
  for kmax in (0, -1, 131073, 1 << 30):
    assert query(kmax) == 0, kmax


def test_cpu_tensors_and_bad_arguments_are_refused():
  import torch
  import vtc_hip
  from utils import index_coding
  from utils import vector_quantization
  tables = truth.frequencies([5, 1, 0, 9])
  indices = torch.zeros(3, dtype=torch.int32)
  packed = torch.zeros(512, dtype=torch.uint8)
  offsets = torch.zeros(2, dtype=torch.int64)
  with pytest.raises(vtc_hip.VtcHipError):
    index_coding.index_ans_split_stream_bytes(indices, tables)
  with pytest.raises(vtc_hip.VtcHipError):
    index_coding.pack_index_ans_split(indices, tables)
  with pytest.raises(vtc_hip.VtcHipError):
    index_coding.unpack_index_ans_split(packed, offsets, tables, 3, 3)
  with pytest.raises(ValueError):
    index_coding.index_ans_split_frequencies([1, 2, 3], k=4)
  with pytest.raises(ValueError):
    index_coding.index_ans_split_frequencies([1, -2, 3])
  with pytest.raises(ValueError):
    index_coding.index_ans_split_frequencies([[1, 2], [3, 4]])
  with pytest.raises(NotImplementedError):
    index_coding.index_ans_split_frequencies([0] * 131073)
  # the scalar-only entries do not know the name
  with pytest.raises(ValueError):
    vector_quantization.compute_RD_point(None, None, None, None,
                                         source_code='ans_split')


# -------------------------------------------------------------- frequencies
def _both(counts, k=None):
  """The product's tables, checked against the restatement's and the model."""
  from utils import index_coding
  freq_hi, freq_lo = index_coding.index_ans_split_frequencies(counts, k)
  want_hi, want_lo = truth.frequencies(counts, k)
  kmax = len(counts)
  k = kmax if k is None else k
  assert freq_hi.dtype == freq_lo.dtype == np.uint16
  assert freq_hi.shape == (truth.hi_symbols(kmax),)
  assert freq_lo.shape == (truth.hi_symbols(kmax), LO)
  assert np.array_equal(freq_hi, want_hi) and np.array_equal(freq_lo, want_lo)
  assert truth.bad_table(freq_hi, freq_lo, kmax) == 0
  # every index below k is codable, none from k on
  flat = freq_lo.reshape(-1)
  present = (freq_hi[np.arange(len(flat)) >> truth.LO_BITS] > 0) & (flat > 0)
  assert present[:k].all() and not present[k:].any()
  return freq_hi.tolist(), freq_lo.tolist()


def test_frequencies_follow_the_rule():
  # k = 1: both tables hold one symbol of frequency 2^15
  hi, lo = _both([7])
  assert hi == [SCALE] and lo == [[SCALE] + [0] * 255]
  hi, lo = _both([7, 3, 3, 3], 1)
  assert hi == [SCALE] and lo == [[SCALE] + [0] * 255]
  # k = 256: one full block
  hi, lo = _both([0] * 256)
  assert hi == [SCALE] and lo == [[128] * 256]
  # k = 257: block weights 256 and 1 -> floor(256 * 2^15 / 257) = 32640 and
  # floor(2^15 / 257) = 127; the one unit left goes to the heavier block
  hi, lo = _both([0] * 257)
  assert hi == [32641, 127]
  assert lo == [[128] * 256, [SCALE] + [0] * 255]
  # k = kmax = 131072, every count 0
  hi, lo = _both([0] * 131072)
  assert hi == [64] * 512 and lo == [[128] * 256] * 512
  # a dominant zero codeword, k = kmax = 1000: block weights 10^9 + 255, 256,
  # 256, 232; the light blocks floor to 0 -> 1, the heavy one to 32767, and
  # the two units too many are taken from the only block above 1
  hi, lo = _both([10 ** 9] + [0] * 999)
  assert hi == [SCALE - 3, 1, 1, 1]
  assert lo[0] == [SCALE - 255] + [1] * 255
  assert lo[1] == lo[2] == [128] * 256
  # 2^15 = 232 * 141 + 56
  assert lo[3] == [142] * 56 + [141] * 176 + [0] * 24
  # k < kmax: the blocks past k are all zero and have hi frequency 0
  hi, lo = _both([3] * 600, 300)
  assert hi[2] == 0 and lo[2] == [0] * 256 and lo[1][44:] == [0] * 212
  rs = np.random.RandomState(3)
  _both(rs.randint(0, 50, size=5000).tolist(), 4097)
  _both(rs.randint(0, 3, size=70000).tolist())


# -------------------------------------------------------------- restatement
def test_restatement_on_hand_worked_cases():
  # hi and lo each of two symbols at 2^14: two bits an index; 64 x 9 indices
  # take a lane from 2^16 past 2^32 once: 64 words
  freq_hi = np.array([1 << 14, 1 << 14], np.uint16)
  freq_lo = np.zeros((2, LO), np.uint16)
  freq_lo[:, :2] = 1 << 14
  host = np.zeros(64 * 9, np.int32)
  streams, status = truth.encode(host, freq_hi, freq_lo, 2 * LO, 64 * 9)
  assert status == [0, 0, 0] and len(streams[0]) == truth.HEADER + 2 * 64
  # a one-symbol hi with a one-symbol lo costs nothing
  tables = truth.hand_tables()
  freq_hi, freq_lo, kmax, host = tables['single']
  streams, status = truth.encode(host, freq_hi, freq_lo, kmax, 200)
  assert streams == [(truth.LOWER).to_bytes(4, 'little') * 64]
  # all four kinds of uncodable entries
  freq_hi, freq_lo, kmax, _ = tables['lo-gap']
  host = np.array([3, -1, kmax, 1, 2, 200], np.int32)
  assert truth.encode(host, freq_hi, freq_lo, kmax, 4)[1] == [3, 2, 0]
  freq_hi, freq_lo, kmax, _ = tables['hi-gap']
  host = np.array([5, 600, 256 + 5, 511], np.int32)
  assert truth.encode(host, freq_hi, freq_lo, kmax, 4)[1] == [2, 3, 0]
  # bad tables: the hi sum first, then the smallest bad row in use
  freq_hi, freq_lo, kmax, host = tables['partial']
  wrong = freq_hi.copy()
  wrong[0] += 1
  bad_lo = freq_lo.copy()
  bad_lo[3, 0] += 1
  bad_lo[1, 9] -= 1
  past = freq_lo.copy()
  past[4, 4] -= 1
  past[4, 5] += 1              # 256 * 4 + 5 = kmax
  for fh, fl, word in ((wrong, bad_lo, 1), (freq_hi, bad_lo, 2 + 1),
                       (freq_hi, past, 2 + 4)):
    streams, status = truth.encode(host, fh, fl, kmax, 64)
    assert streams == [b''] * 4 and status == [0, 0, word]
    got, used, status = truth.decode(np.zeros(9, np.uint8), [0] * 5, 200, fh,
                                     fl, kmax, 64)
    assert (got == -1).all() and (used == 0).all() and status == [0, 0, word]
  # the same row beyond a larger kmax is fine
  assert truth.bad_table(freq_hi, past, kmax + 1) == 0


def _round_trip(host, freq_hi, freq_lo, kmax, rows):
  b = len(host)
  streams, status = truth.encode(host, freq_hi, freq_lo, kmax, rows)
  assert status == [0, 0, 0]
  n = truth.streams_of(b, rows)
  assert len(streams) == n
  assert all(len(s) >= truth.HEADER and len(s) % 2 == 0 for s in streams)
  sizes = [len(s) for s in streams]
  for lead in (0, 3):
    offsets = truth.layout(sizes, lead, truth.gaps(n))
    packed, skipped = truth.image(streams, offsets, int(offsets[-1]))
    assert skipped == 0
    got, used, status = truth.decode(packed, offsets, b, freq_hi, freq_lo,
                                     kmax, rows)
    assert status == [0, 0, 0]
    assert np.array_equal(got, host) and used.tolist() == sizes
  return sizes


@pytest.mark.parametrize('case', truth.CASES, ids=truth.IDS)
def test_restatement_round_trips_every_case(case):
  b, kmax, rows = case
  freq_hi, freq_lo = truth.case_tables(*case)
  host = truth.case_indices(*case)
  assert len(host) == b and host.max() < kmax
  _round_trip(host, freq_hi, freq_lo, kmax, rows)
  assert [len(s) for s in truth.case_streams(*case)] == _round_trip(
      host, freq_hi, freq_lo, kmax, rows)


@pytest.mark.parametrize('name', sorted(truth.hand_tables()))
def test_restatement_round_trips_hand_made_tables(name):
  freq_hi, freq_lo, kmax, host = truth.hand_tables()[name]
  assert truth.bad_table(freq_hi, freq_lo, kmax) == 0
  for rows in (64, 100, 1000):
    sizes = _round_trip(host, freq_hi, freq_lo, kmax, rows)
    if name == 'single':
      assert set(sizes) == {truth.HEADER}


@pytest.mark.parametrize('scene', truth.SCENES,
                         ids=['%d-k%d-kmax%d-z%g' % s for s in truth.SCENES])
def test_cost_stays_within_the_flush_of_the_ideal(scene):
  """8 x bytes >= ideal and <= ideal + n (8 * 256 + 16) + 0.01 ideal, the
  bound tests/test_index_ans_host.py puts on the one-table coder."""
  b, k, kmax, p_zero = scene
  rows = 65536
  host = truth.sparse_indices(11, b, k, p_zero)
  freq_hi, freq_lo = truth.frequencies(
      np.bincount(host, minlength=kmax).tolist(), k)
  streams, status = truth.encode(host, freq_hi, freq_lo, kmax, rows)
  assert status == [0, 0, 0]
  n = truth.streams_of(b, rows)
  sizes = [len(s) for s in streams]
  offsets = truth.layout(sizes, 0, [0] * n)
  packed, _ = truth.image(streams, offsets, int(offsets[-1]))
  got, used, status = truth.decode(packed, offsets, b, freq_hi, freq_lo, kmax,
                                   rows)
  assert status == [0, 0, 0] and np.array_equal(got, host)
  assert used.tolist() == sizes
  ideal = truth.ideal_bits(host, freq_hi, freq_lo)
  entropy = truth.entropy_bits(host, kmax)
  coded = 8 * sum(sizes)
  print('index_ans_split_rate per index: entropy %.4f ideal %.4f coded %.4f'
        % (entropy / b, ideal / b, coded / float(b)))
  assert ideal >= entropy
  assert coded >= ideal
  assert coded <= ideal + n * (8 * truth.HEADER + 16) + 0.01 * ideal


def test_restatement_classifies_damaged_streams():
  case = (300, 5000, 100)
  b, kmax, rows = case
  freq_hi, freq_lo = truth.case_tables(*case)
  host = truth.case_indices(*case)
  streams = truth.case_streams(*case)
  sizes = [len(s) for s in streams]
  offsets = truth.layout(sizes, 0, [0, 0, 0])
  packed, _ = truth.image(streams, offsets, int(offsets[-1]))
  args = (b, freq_hi, freq_lo, kmax, rows)
  # the middle slot cut by two bytes: it runs dry in its last steps
  shifted = np.concatenate([packed[:offsets[2] - 2], packed[offsets[2]:]])
  moved = np.array([offsets[0], offsets[1], offsets[2] - 2, offsets[3] - 2])
  got, used, status = truth.decode(shifted, moved, *args)
  assert status == [1, 2, 0]
  assert np.array_equal(got[:100], host[:100])
  assert np.array_equal(got[200:], host[200:])
  middle = got[100:200]
  dry = np.nonzero(middle < 0)[0]
  assert len(dry) and dry[0] % 64 == 0 and (middle[dry[0]:] == -1).all()
  assert np.array_equal(middle[:dry[0]], host[100:200][:dry[0]])
  assert used[1] < sizes[1] and (used[1] - truth.HEADER) % 2 == 0
  # one flipped word: everything decodes to something, the end states tell
  flipped = packed.copy()
  flipped[offsets[1] + truth.HEADER + 10] ^= 0x40
  got, used, status = truth.decode(flipped, offsets, *args)
  assert status[:2] == [1, 2]
  assert np.array_equal(got[:100], host[:100])
  assert np.array_equal(got[200:], host[200:])
  assert ((got[100:200] >= -1) & (got[100:200] < kmax)).all()
  # offsets that decrease; a negative one; a buffer ending inside the states
  wrong = offsets.copy()
  wrong[1] = offsets[2] + 4
  got, used, status = truth.decode(packed, wrong, *args)
  assert status[1] in (1, 2) and (got[100:200] == -1).all() and used[1] == 0
  wrong = offsets.copy()
  wrong[0] = -2
  got, used, status = truth.decode(packed, wrong, *args)
  assert status == [1, 1, 0] and (got[:100] == -1).all() and used[0] == 0
  short = packed[:offsets[2] + 100]
  got, used, status = truth.decode(short, offsets, *args)
  assert status == [1, 3, 0] and (got[200:] == -1).all() and used[2] == 0
  assert np.array_equal(got[:200], host[:200])
