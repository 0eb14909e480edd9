"""The twelfth header, include/vtc_vq_large.h, held to what
tests/test_vq_host.py asks of the eighth: VQ_LARGE_SIGNATURES is exactly the
declared surface and shares no name with the other eleven headers, the library
exports it, both ABI versions, the workspace query term for term and under
64 MiB at the experiment's shape, bad arguments answered before any device
work; the host rule of initial_vector_codebook with max_codewords against the
restatement of tests/vq_large_data.py, and the defaults of today.  No GPU
needed."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import vq_data as small
import vq_large_data as data

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'vtc_vq_large.h'
OTHER_HEADERS = sorted(path for path in (REPO / 'include').glob('*.h')
                       if path != HEADER)

OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, 1, 2, 3
ENTRY_POINTS = ['vtc_vq_large_abi_version', 'vtc_vq_large_assign',
                'vtc_vq_large_index_counts', 'vtc_vq_large_lloyd_step',
                'vtc_vq_large_lloyd_step_workspace_bytes']


def _code(path):
  return re.sub(r'/\*.*?\*/', '', path.read_text(), flags=re.S)


def declarations(path=HEADER):
  """name -> argument text of every function the header declares."""
  return {m.group(1): m.group(2)
          for m in re.finditer(r'\b(vtc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;',
                               _code(path))}


def _lib():
  import vtc_hip
  return vtc_hip, vtc_hip.load_library()


def test_header_is_parsed():
  assert sorted(declarations()) == ENTRY_POINTS
  code = _code(HEADER)
  assert re.search(r'#define\s+VTC_VQ_LARGE_ABI_VERSION\s+1\b', code)
  assert re.search(r'#define\s+VTC_VQ_LARGE_MAX_CODEWORDS\s+%d\b'
                   % data.MAX_CODEWORDS, code)
  assert data.MAX_CODEWORDS == 131072 == 1 << 17
  assert '#include "vtc_vq.h"' in code
  assert 'struct' not in code          # vtc_vq_state is the eighth header's
  # every function has the argument list of its twin of the eighth header
  twins = declarations(REPO / 'include' / 'vtc_vq.h')
  for name, args in declarations().items():
    twin = twins[name.replace('vtc_vq_large_', 'vtc_vq_')]
    assert re.sub(r'\s+', ' ', args) == re.sub(r'\s+', ' ', twin), name
  # what the comment has to say about skipped blocks
  text = HEADER.read_text()
  assert 'skipped' in text and '+0.0' in text


def test_the_twelve_headers_do_not_overlap():
  assert len(OTHER_HEADERS) == 11
  for other in OTHER_HEADERS:
    names = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(other)))
    assert names and not names & set(declarations()), other.name


def test_binding_table_is_the_declared_surface():
  vtc_hip, lib = _lib()
  assert sorted(vtc_hip.VQ_LARGE_SIGNATURES) == sorted(declarations())
  tables = [getattr(vtc_hip, name) for name in dir(vtc_hip)
            if name.endswith('SIGNATURES') and name != 'VQ_LARGE_SIGNATURES']
  assert len(tables) == 11
  for other in tables:
    assert not set(vtc_hip.VQ_LARGE_SIGNATURES) & set(other)
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declarations().items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.VQ_LARGE_SIGNATURES[name][1]) == count, name
    assert getattr(lib, name).argtypes == vtc_hip.VQ_LARGE_SIGNATURES[name][1]
    twin = name.replace('vtc_vq_large_', 'vtc_vq_')
    assert vtc_hip.VQ_LARGE_SIGNATURES[name] == vtc_hip.VQ_SIGNATURES[twin]
  assert lib.vtc_vq_large_abi_version() == vtc_hip.VQ_LARGE_ABI_VERSION == 1
  assert vtc_hip.VQ_LARGE_MAX_CODEWORDS == data.MAX_CODEWORDS
  # the eighth header stays where it was
  assert lib.vtc_vq_abi_version() == vtc_hip.VQ_ABI_VERSION == 1
  assert len(vtc_hip.VQ_SIGNATURES) == 5
  assert vtc_hip.VQ_MAX_CODEWORDS == small.MAX_CODEWORDS == 4096


def test_workspace_query_is_stated_term_for_term():
  _, lib = _lib()
  query = lib.vtc_vq_large_lloyd_step_workspace_bytes
  for b, d, kmax in ((1, 1, 1), (257, 23, 40), (2 * data.ROWS + 3, 23, 200),
                     (65, 32, 4096), (4099, 23, 4097), (100000, 23, 4096),
                     (100000, 23, 131072), (100000, 32, 131072),
                     (1 << 33, 2, 7)):
    assert query(b, d, kmax) == data.workspace_formula(b, d, kmax), (b, d,
                                                                      kmax)
  # the experiment's shape: under 64 MiB, the per-block part at most
  # ceil(b / 2048) * 2048 * (d + 3) eight-byte words
  assert query(100000, 23, 131072) < 64 << 20
  c = -(-100000 // data.ROWS)
  per_block = sum(data.padded(n * data.ROWS * c) for n in (4, 8 * 23, 8, 4))
  assert per_block + data.padded(4 * c) <= 8 * c * data.ROWS * (23 + 3)
  # nothing grows with c * kmax: doubling kmax adds the four per-cell arrays
  assert (query(100000, 23, 131072) - query(100000, 23, 65536) ==
          (8 + 8 + 8 + 4) * 65536)
  for b, d, kmax in ((0, 4, 4), (-1, 4, 4), (4, 0, 4), (4, 33, 4), (4, 4, 0),
                     (4, 4, -1), (4, 4, 131073), (1 << 41, 4, 4)):
    assert query(b, d, kmax) == 0, (b, d, kmax)
  # the eighth header's query still stops at 4096
  assert lib.vtc_vq_lloyd_step_workspace_bytes(4, 4, 4097) == 0


def _refused(lib, rc, status, *words):
  assert rc == status, (rc, lib.vtc_last_error())
  text = lib.vtc_last_error().decode()
  for word in words:
    assert word in text, text


def _state(vtc_hip, base, skip=None):
  fields = [f[0] for f in vtc_hip.VqState._fields_]
  return vtc_hip.VqState(**{name: (0 if name == skip else (base + n) << 20)
                            for n, name in enumerate(fields)})


def test_argument_errors_do_not_touch_the_gpu():
  """Null pointers, bad sizes, unsupported sizes and a short or missing
  workspace, one argument at a time.  The non-null pointers are host integers
  that are never dereferenced: this runs with no device."""
  vtc_hip, lib = _lib()
  p = [ctypes.c_void_p(v << 20) for v in range(1, 12)]

  who = 'vtc_vq_large_assign'
  #       vectors b   d   book  lens  k    kmax   lam indices deq status stream
  good = [p[0], 257, 23, p[1], p[2], p[3], 5000, 0.5, p[4], p[5], p[6], None]
  for position in (0, 3, 5, 8, 10):
    args = list(good)
    args[position] = None
    _refused(lib, lib.vtc_vq_large_assign(*args), ERR_INVALID_ARGUMENT, who,
             'null')
  args = list(good)
  args[4] = None   # lengths are needed when lambda != 0
  _refused(lib, lib.vtc_vq_large_assign(*args), ERR_INVALID_ARGUMENT, who,
           'null', 'lengths')
  for position, value, word in ((1, 0, 'b = 0'), (1, -3, 'b = -3'),
                                (2, 0, 'd = 0'), (6, 0, 'kmax = 0'),
                                (7, -1.0, 'lambda'),
                                (7, float('nan'), 'lambda')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_vq_large_assign(*args), ERR_INVALID_ARGUMENT, who,
             word)
  for position, value, words in ((2, 33, ('d = 33', 'at most 32')),
                                 (6, 131073, ('kmax = 131073',
                                              'at most 131072'))):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_vq_large_assign(*args), ERR_UNSUPPORTED, who, *words)

  who = 'vtc_vq_large_lloyd_step'
  need = lib.vtc_vq_large_lloyd_step_workspace_bytes(257, 23, 5000)
  assert need > 0
  state_in, state_out = _state(vtc_hip, 20), _state(vtc_hip, 40)
  #       vectors b   d  kmax  lam  eps  pin in  out  status ws  bytes stream
  good = [p[0], 257, 23, 5000, 0.5, 1e-5, 1, ctypes.byref(state_in),
          ctypes.byref(state_out), p[1], p[2], need, None]
  for position in (0, 7, 8, 9):
    args = list(good)
    args[position] = None
    _refused(lib, lib.vtc_vq_large_lloyd_step(*args), ERR_INVALID_ARGUMENT,
             who, 'null')
  for field, _ in vtc_hip.VqState._fields_:
    for position, word in ((7, '(in)'), (8, '(out)')):
      args = list(good)
      args[position] = ctypes.byref(_state(vtc_hip, 60, skip=field))
      _refused(lib, lib.vtc_vq_large_lloyd_step(*args), ERR_INVALID_ARGUMENT,
               who, 'null', word)
  for position, value, word in ((1, 0, 'b = 0'), (2, 0, 'd = 0'),
                                (2, -1, 'd = -1'), (3, 0, 'kmax = 0'),
                                (4, -0.5, 'lambda'),
                                (4, float('nan'), 'lambda')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_vq_large_lloyd_step(*args), ERR_INVALID_ARGUMENT,
             who, word)
  for position, value, words in ((2, 33, ('d = 33', 'at most 32')),
                                 (3, 131073, ('kmax = 131073',
                                              'at most 131072'))):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_vq_large_lloyd_step(*args), ERR_UNSUPPORTED, who,
             *words)
  args = list(good)
  args[11] = need - 1
  _refused(lib, lib.vtc_vq_large_lloyd_step(*args), ERR_WORKSPACE, who,
           'workspace', '%d bytes, %d needed' % (need - 1, need))
  args = list(good)
  args[10] = None
  _refused(lib, lib.vtc_vq_large_lloyd_step(*args), ERR_WORKSPACE, who,
           'workspace')
  # 131072 codewords of 32 components are supported: this gets as far as the
  # workspace check
  args = list(good)
  args[2], args[3], args[11] = 32, 131072, 0
  _refused(lib, lib.vtc_vq_large_lloyd_step(*args), ERR_WORKSPACE, who,
           'workspace')

  who = 'vtc_vq_large_index_counts'
  #       indices b   kmax  counts stream
  good = [p[0], 257, 5000, p[1], None]
  for position in (0, 3):
    args = list(good)
    args[position] = None
    _refused(lib, lib.vtc_vq_large_index_counts(*args), ERR_INVALID_ARGUMENT,
             who, 'null')
  for position, value, word in ((1, 0, 'b = 0'), (2, -2, 'kmax = -2')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_vq_large_index_counts(*args), ERR_INVALID_ARGUMENT,
             who, word)
  args = list(good)
  args[2] = 131073
  _refused(lib, lib.vtc_vq_large_index_counts(*args), ERR_UNSUPPORTED, who,
           'kmax = 131073', 'at most 131072')


def test_initial_codebook_with_max_codewords():
  """The host half of initial_vector_codebook against the restatement, at the
  default cap (today's array) and above it."""
  from utils import vector_quantization as vq
  assert vq.VQ_LARGE_MAX_CODEWORDS == data.MAX_CODEWORDS
  x = np.array([[1.0, 2.0], [0.0, -0.0], [1.0, 2.0], [np.nan, 3.0],
                [-0.0, 5.0], [0.0, 5.0], [4.0, 4.0], [0.0, 0.0]], np.float32)
  want = np.array([[0.0, 0.0], [1.0, 2.0], [0.0, 5.0], [4.0, 4.0]])
  for cap in (4096, 131072):
    for make in (data.initial_codebook, vq._initial_codebook_host):
      got = make(x, 100, cap)
      assert got.dtype == np.float64 and np.array_equal(got, want)
      assert not np.signbit(got).any()
  for make in (data.initial_codebook, vq._initial_codebook_host):
    assert np.array_equal(make(x, 100, 3), want[:3])    # at most 3 rows
  # 5000 distinct rows: 4096 candidates by default, all of them when asked
  big = np.arange(1, 5001, dtype=np.float32)[:, None] * np.ones((1, 2),
                                                                np.float32)
  today = small.initial_codebook(big, 100000)
  assert today.shape == (4096, 2)
  for make in (data.initial_codebook, vq._initial_codebook_host):
    assert np.array_equal(make(big, 100000), today)           # the default
    assert np.array_equal(make(big, 100000, 4096), today)
    got = make(big, 100000, 131072)
    assert got.shape == (5001, 2) and (got[0] == 0).all()
    assert np.array_equal(got[1:, 0], big[:, 0])
    got = make(big, 100000, 4500)                  # 4500 candidates: rows
    picked = (np.arange(4500) * 5000) // 4500      # floor(i * b / m)
    assert got.shape == (4500, 2)
    assert np.array_equal(got[1:, 0], big[picked[:4499], 0])
  # seeded data with duplicates (zero rows) and a cap in between
  x = small.vectors(77, 6000, 5)
  for cap in (4096, 5000, 131072):
    assert np.array_equal(data.initial_codebook(x, 100000, cap),
                          vq._initial_codebook_host(x, 100000, cap)), cap
  assert np.array_equal(vq._initial_codebook_host(x, 100000),
                        small.initial_codebook(x, 100000))
  for bad in (0, -1, 131073):
    with pytest.raises(ValueError, match='max_codewords'):
      vq._initial_codebook_host(x, 100, bad)


def test_python_surface_and_defaults():
  """The new keywords exist, default to 4096, and the table codes refuse a
  codebook of more than 4096 slots before anything touches a device."""
  import inspect
  import torch
  from utils import vector_quantization as vq
  for name, keyword in (('initial_vector_codebook', 'max_codewords'),
                        ('vector_assign', 'max_codewords'),
                        ('vector_index_counts', 'max_codewords'),
                        ('vector_dequantize', 'max_codewords'),
                        ('vector_lloyd', 'max_codewords'),
                        ('compute_RD_point_mixed', 'vec_max_codewords'),
                        ('Mod2_compute_RD_point', 'vec_max_codewords'),
                        ('Mod3_compute_RD_point', 'vec_max_codewords')):
    parameter = inspect.signature(getattr(vq, name)).parameters[keyword]
    assert parameter.default == 4096 == vq.VQ_MAX_CODEWORDS, name
  assert callable(vq.trim_vector_codebook)
  # CPU tensors: the check of the table code comes before the device check
  codes, patches, dictionary = (torch.zeros(8, 4), torch.zeros(8, 6),
                                torch.zeros(4, 6))
  scal = (np.zeros((1, 1)), np.ones(1, np.int32))
  for source_code in ('huffman', 'ans'):
    with pytest.raises(NotImplementedError, match='trim_vector_codebook'):
      vq.compute_RD_point_mixed(codes, patches, dictionary, [0], scal,
                                [1, 2, 3], np.zeros((4097, 3)),
                                source_code=source_code,
                                vec_max_codewords=131072)
  import vtc_hip
  with pytest.raises(vtc_hip.VtcHipError):      # 'entropy' gets to the device
    vq.compute_RD_point_mixed(codes, patches, dictionary, [0], scal,
                              [1, 2, 3], np.zeros((4097, 3)),
                              vec_max_codewords=131072)
