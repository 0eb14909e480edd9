"""The eighth header, include/vtc_vq.h, held to what
tests/test_quantization_host.py asks of the seventh: VQ_SIGNATURES is exactly
the declared surface and shares no name with the other seven tables, the
library exports it, the workspace query term for term, bad arguments answered
before any device work; utils.vector_quantization is a superset of
utils.quantization; the numpy restatement of tests/vq_data.py against a
brute-force loop, its initial codebook, the conditions that keep
tests/golden/vq.npz discriminating, and the fixture against a fresh run.  No
GPU needed."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import helpers
import vq_data as data

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'vtc_vq.h'
OTHER_HEADERS = [REPO / 'include' / name
                 for name in ('vtc_hip.h', 'vtc_image.h', 'vtc_codec.h',
                              'vtc_decode.h', 'vtc_quality.h', 'vtc_stats.h',
                              'vtc_quant.h')]

OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, 1, 2, 3


def _code(path):
  return re.sub(r'/\*.*?\*/', '', path.read_text(), flags=re.S)


def declarations():
  """name -> argument text of every function include/vtc_vq.h declares."""
  return {m.group(1): m.group(2)
          for m in re.finditer(r'\b(vtc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;',
                               _code(HEADER))}


def _lib():
  import vtc_hip
  return vtc_hip, vtc_hip.load_library()


def padded(nbytes):
  return -(-nbytes // 256) * 256


def test_header_is_parsed():
  assert sorted(declarations()) == [
      'vtc_vq_abi_version', 'vtc_vq_assign', 'vtc_vq_index_counts',
      'vtc_vq_lloyd_step', 'vtc_vq_lloyd_step_workspace_bytes']
  code = _code(HEADER)
  for name, value in (('ABI_VERSION', 1), ('MAX_DIM', data.MAX_DIM),
                      ('MAX_CODEWORDS', data.MAX_CODEWORDS),
                      ('ASSIGN_ROWS', data.ASSIGN_ROWS),
                      ('TILE_DOUBLES', data.TILE_DOUBLES),
                      ('ROWS', data.ROWS)):
    assert re.search(r'#define\s+VTC_VQ_%s\s+%d\b' % (name, value), code), name
  assert (data.MAX_DIM, data.MAX_CODEWORDS) == (32, 4096)
  assert '#include "vtc_quality.h"' in code
  assert data.tile_codewords(23) == 170 and data.tile_codewords(32) == 128


def test_the_eight_headers_do_not_overlap():
  for other in OTHER_HEADERS:
    names = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(other)))
    assert names and not names & set(declarations()), other.name


def test_binding_table_is_the_declared_surface():
  vtc_hip, lib = _lib()
  assert sorted(vtc_hip.VQ_SIGNATURES) == sorted(declarations())
  for other in (vtc_hip.SIGNATURES, vtc_hip.IMAGE_SIGNATURES,
                vtc_hip.CODEC_SIGNATURES, vtc_hip.DECODE_SIGNATURES,
                vtc_hip.QUALITY_SIGNATURES, vtc_hip.STATS_SIGNATURES,
                vtc_hip.QUANT_SIGNATURES):
    assert not set(vtc_hip.VQ_SIGNATURES) & set(other)
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declarations().items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.VQ_SIGNATURES[name][1]) == count, name
    assert getattr(lib, name).argtypes == vtc_hip.VQ_SIGNATURES[name][1]
  assert lib.vtc_vq_abi_version() == vtc_hip.VQ_ABI_VERSION == 1
  assert (vtc_hip.VQ_MAX_DIM, vtc_hip.VQ_MAX_CODEWORDS, vtc_hip.VQ_ROWS,
          vtc_hip.VQ_TILE_DOUBLES) == (data.MAX_DIM, data.MAX_CODEWORDS,
                                       data.ROWS, data.TILE_DOUBLES)
  # struct vtc_vq_state: eight pointers in the header's order
  fields = re.search(r'typedef struct vtc_vq_state \{(.*?)\}', _code(HEADER),
                     flags=re.S).group(1)
  assert [f[0] for f in vtc_hip.VqState._fields_] == re.findall(
      r'\*\s*(\w+)\s*;', fields)
  assert ctypes.sizeof(vtc_hip.VqState) == 8 * ctypes.sizeof(ctypes.c_void_p)
  # the seventh header stays where it was
  assert lib.vtc_quant_abi_version() == 1
  assert len(vtc_hip.QUANT_SIGNATURES) == 5


def workspace_formula(b, d, kmax):
  c = -(-b // data.ROWS)
  return (padded(4 * b) + padded(8 * b) + padded(8 * c * kmax * d) +
          padded(8 * c * kmax) + padded(4 * c * kmax) + padded(8 * kmax) +
          padded(4 * kmax) + 256 + 256)


def test_workspace_query_is_stated_term_for_term():
  _, lib = _lib()
  for b, d, kmax in ((1, 1, 1), (257, 23, 40), (2 * data.ROWS + 3, 23, 200),
                     (65, 32, 4096), (100000, 23, 4096), (1 << 33, 2, 7)):
    assert lib.vtc_vq_lloyd_step_workspace_bytes(b, d, kmax) == (
        workspace_formula(b, d, kmax)), (b, d, kmax)
  # the experiment's shape: a small fraction of device memory
  assert workspace_formula(100000, 23, 4096) < 64 << 20
  for b, d, kmax in ((0, 4, 4), (-1, 4, 4), (4, 0, 4), (4, 33, 4), (4, 4, 0),
                     (4, 4, 4097), (1 << 41, 4, 4)):
    assert lib.vtc_vq_lloyd_step_workspace_bytes(b, d, kmax) == 0


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

  who = 'vtc_vq_assign'
  #       vectors b   d   book  lens  k    kmax lam indices deq  status stream
  good = [p[0], 257, 23, p[1], p[2], p[3], 40, 0.5, p[4], p[5], p[6], None]
  for position in (0, 3, 5, 8, 10):
    args = list(good)
    args[position] = None
    _refused(lib, lib.vtc_vq_assign(*args), ERR_INVALID_ARGUMENT, who, 'null')
  args = list(good)
  args[4] = None   # lengths are needed when lambda != 0
  _refused(lib, lib.vtc_vq_assign(*args), ERR_INVALID_ARGUMENT, who, 'null',
           'lengths')
  for position, value, word in ((1, 0, 'b = 0'), (1, -3, 'b = -3'),
                                (2, 0, 'd = 0'), (6, 0, 'kmax = 0'),
                                (7, -1.0, 'lambda'),
                                (7, float('nan'), 'lambda')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_vq_assign(*args), ERR_INVALID_ARGUMENT, who, word)
  for position, value, word in ((2, 33, 'd = 33'), (6, 4097, 'kmax = 4097')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_vq_assign(*args), ERR_UNSUPPORTED, who, word)

  who = 'vtc_vq_lloyd_step'
  need = lib.vtc_vq_lloyd_step_workspace_bytes(257, 23, 40)
  assert need > 0
  state_in, state_out = _state(vtc_hip, 20), _state(vtc_hip, 40)
  #       vectors b   d  kmax lam  eps  pin in  out  status ws  bytes stream
  good = [p[0], 257, 23, 40, 0.5, 1e-5, 1, ctypes.byref(state_in),
          ctypes.byref(state_out), p[1], p[2], need, None]
  for position in (0, 7, 8, 9):
    args = list(good)
    args[position] = None
    _refused(lib, lib.vtc_vq_lloyd_step(*args), ERR_INVALID_ARGUMENT, who,
             'null')
  for field, _ in vtc_hip.VqState._fields_:
    for position, word in ((7, '(in)'), (8, '(out)')):
      args = list(good)
      args[position] = ctypes.byref(_state(vtc_hip, 60, skip=field))
      _refused(lib, lib.vtc_vq_lloyd_step(*args), ERR_INVALID_ARGUMENT, who,
               'null', word)
  for position, value, word in ((1, 0, 'b = 0'), (2, 0, 'd = 0'),
                                (2, -1, 'd = -1'), (3, 0, 'kmax = 0'),
                                (4, -0.5, 'lambda'),
                                (4, float('nan'), 'lambda')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_vq_lloyd_step(*args), ERR_INVALID_ARGUMENT, who,
             word)
  for position, value, word in ((2, 33, 'd = 33'), (3, 4097, 'kmax = 4097')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_vq_lloyd_step(*args), ERR_UNSUPPORTED, who, word)
  args = list(good)
  args[11] = need - 1
  _refused(lib, lib.vtc_vq_lloyd_step(*args), ERR_WORKSPACE, who,
           'workspace', '%d bytes, %d needed' % (need - 1, need))
  args = list(good)
  args[10] = None
  _refused(lib, lib.vtc_vq_lloyd_step(*args), ERR_WORKSPACE, who, 'workspace')
  # 4096 codewords of 32 components are supported: this gets as far as the
  # workspace check
  args = list(good)
  args[2], args[3], args[11] = 32, 4096, 0
  _refused(lib, lib.vtc_vq_lloyd_step(*args), ERR_WORKSPACE, who, 'workspace')

  who = 'vtc_vq_index_counts'
  #       indices b   kmax counts stream
  good = [p[0], 257, 40, p[1], None]
  for position in (0, 3):
    args = list(good)
    args[position] = None
    _refused(lib, lib.vtc_vq_index_counts(*args), ERR_INVALID_ARGUMENT, who,
             'null')
  for position, value, word in ((1, 0, 'b = 0'), (2, -2, 'kmax = -2')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_vq_index_counts(*args), ERR_INVALID_ARGUMENT, who,
             word)
  args = list(good)
  args[2] = 4097
  _refused(lib, lib.vtc_vq_index_counts(*args), ERR_UNSUPPORTED, who,
           'kmax = 4097')


def test_module_is_a_superset_of_utils_quantization():
  from utils import quantization
  from utils import vector_quantization
  public = [name for name in dir(quantization) if not name.startswith('_')]
  assert 'Mod1_compute_RD_point' in public and 'scalar_lloyd' in public
  for name in public:
    assert getattr(vector_quantization, name) is getattr(quantization, name)
  for name in ('vector_assign', 'vector_dequantize', 'vector_index_counts',
               'initial_vector_codebook', 'vector_lloyd',
               'compute_RD_point_mixed', 'Mod2_compute_RD_point',
               'Mod3_compute_RD_point'):
    assert callable(getattr(vector_quantization, name)), name
    assert not hasattr(quantization, name), name


def test_cpu_tensors_are_refused():
  import torch
  import vtc_hip
  from utils import vector_quantization as vq
  x = torch.zeros(8, 3)
  book = np.zeros((1, 3))
  with pytest.raises(vtc_hip.VtcHipError):
    vq.vector_assign(x, book)
  with pytest.raises(vtc_hip.VtcHipError):
    vq.vector_lloyd(x, book)
  with pytest.raises(vtc_hip.VtcHipError):
    vq.initial_vector_codebook(x, 4)
  with pytest.raises(vtc_hip.VtcHipError):
    vq.vector_index_counts(torch.zeros(8, dtype=torch.int32), 4)
  with pytest.raises(vtc_hip.VtcHipError):
    vq.vector_dequantize(torch.zeros(8, dtype=torch.int32), book)
  codes, patches, dictionary = (torch.zeros(8, 4), torch.zeros(8, 6),
                                torch.zeros(4, 6))
  with pytest.raises(vtc_hip.VtcHipError):
    vq.compute_RD_point_mixed(codes, patches, dictionary, [0],
                              (np.zeros((1, 1)), np.ones(1, np.int32)),
                              [1, 2, 3], book)
  for entry in (vq.Mod2_compute_RD_point, vq.Mod3_compute_RD_point):
    with pytest.raises(vtc_hip.VtcHipError):
      entry(codes, patches, dictionary, [0], [1, 2, 3], scal_binwidths=[1.0])
  with pytest.raises(TypeError):
    vq.vector_assign(np.zeros((8, 3), np.float32), book)


def test_restatement_matches_a_brute_force_loop():
  """assign and one step of vq_data on a tiny case against plain Python
  loops that add the components one at a time."""
  rs = np.random.RandomState(4)
  x = rs.randn(11, 3).astype(np.float32)
  x[::3] = 0.0
  book = np.array([[0.0, 0.0, 0.0], [1.0, -0.5, 0.25], [-1.0, 0.5, 0.0],
                   [9.0, 9.0, 9.0], [7.0, 7.0, 7.0]])
  lengths = np.array([1.0, 2.0, 2.5, 3.0, 1.0])
  lam, k = 0.3, 4                     # the fifth slot is past k
  got, _, chosen = data.assign(x, book, k, lengths, lam)
  sums, members, total_d = np.zeros((4, 3)), np.zeros(4, int), 0.0
  for r in range(11):
    best, best_i, best_d = None, -1, None
    for i in range(k):
      dist = 0.0
      for t in range(3):
        e = float(x[r, t]) - book[i, t]
        dist = dist + e * e
      cost = dist + lam * lengths[i]
      if best is None or cost < best:
        best, best_i, best_d = cost, i, dist
    assert got[r] == best_i and chosen[r] == best_d
    sums[best_i] += x[r].astype(np.float64)
    members[best_i] += 1
    total_d += best_d
  state = {'codebook': book, 'lengths': lengths,
           'counts': np.zeros(5, np.int64), 'cost': np.zeros(3),
           'k': np.array([k], np.int32), 'zero_index': np.array([0], np.int32),
           'active': np.ones(1, np.int32), 'iterations': np.zeros(1, np.int32)}
  new, facts = data.step(x, state, lam, 1e-3, True)
  assert members[3] == 0 and facts['lost'] == 1     # 9, 9, 9 has no member
  kept = [i for i in range(k) if members[i] or i == 0]
  assert new['k'][0] == len(kept) and new['zero_index'][0] == 0
  for p, i in enumerate(kept):
    want = np.zeros(3) if i == 0 else sums[i] / members[i]
    assert np.abs(new['codebook'][p] - want).max() <= 1e-15
    assert new['counts'][p] == members[i]
  assert (new['codebook'][len(kept):] == 0).all()
  assert (new['lengths'][len(kept):] == 0).all()
  assert abs(new['cost'][1] - total_d) <= 1e-13 * total_d
  assert new['iterations'][0] == 1 and new['active'][0] == 1
  # a frozen state is returned as it is
  state['active'][0] = 0
  frozen, _ = data.step(x, state, lam, 1e-3, True)
  for key, value in state.items():
    assert np.array_equal(frozen[key], value), key


def test_initial_codebook():
  """Duplicates, -0.0, NaN rows and the cap, in the restatement and in the
  host half of utils.vector_quantization.initial_vector_codebook."""
  from utils import vector_quantization as vq
  x = np.array([[1.0, 2.0], [0.0, -0.0], [1.0, 2.0], [np.nan, 3.0],
                [-0.0, 5.0], [0.0, 5.0], [4.0, 4.0], [0.0, 0.0]], np.float32)
  want = np.array([[0.0, 0.0], [1.0, 2.0], [0.0, 5.0], [4.0, 4.0]])
  for make in (data.initial_codebook, vq._initial_codebook_host):
    got = make(x, 100)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert not np.signbit(got).any()                 # -0.0 became 0.0
    # fewer bins than rows: the rows floor(i * 8 / 3) = 0, 2, 5
    assert np.array_equal(make(x, 3), [[0.0, 0.0], [1.0, 2.0], [0.0, 5.0]])
    assert np.array_equal(make(x[3:4], 5), [[0.0, 0.0]])   # only a NaN row
  # the cap: 5000 distinct rows, 4096 candidates behind the zero vector
  big = np.arange(1, 5001, dtype=np.float32)[:, None] * np.ones((1, 2),
                                                                np.float32)
  for make in (data.initial_codebook, vq._initial_codebook_host):
    got = make(big, 100000)
    assert got.shape == (4096, 2) and (got[0] == 0).all()
    picked = (np.arange(4096) * 5000) // 4096
    assert np.array_equal(got[1:, 0], big[picked[:4095], 0])
  x = data.vectors(77, 300, 5)
  assert np.array_equal(data.initial_codebook(x, 64),
                        vq._initial_codebook_host(x, 64))


def test_fixture_is_discriminating():
  """What tools/make_vq_golden.py asserts, asserted again on a fresh run of
  the restatement, and the stored states and points are that run's: the
  integers equal, the float64 fields within 1e-13 relative (numpy's sums and
  log2 may differ in the last bits between builds and CPUs) -- a hundredth of
  the 1e-11 the GPU tests allow the device."""
  g = helpers.load('vq')
  results = {name: data.run_fit(name) for name in sorted(data.FITS)}
  points = {name: data.rd_point(name) for name in sorted(data.POINTS)}
  facts = data.conditions(results, points)
  data.check_conditions(facts)
  for key, value in facts.items():
    if isinstance(value, (int, np.integer)):
      assert int(g['fact_' + key]) == value, key
    else:   # ratios of small differences: their own last digits may move
      assert np.isclose(float(g['fact_' + key]), value, rtol=1e-4, atol=0), key

  def same_state(prefix, state):
    for key, value in state.items():
      stored = g['%s_%s' % (prefix, key)]
      if key in data.STATE_INT:
        assert np.array_equal(stored, value), (prefix, key)
        continue
      assert np.array_equal(np.isinf(stored), np.isinf(value)), (prefix, key)
      assert not np.isnan(stored).any() and not np.isnan(value).any()
      ok = np.isfinite(value)
      scale = np.maximum(np.abs(value[ok]), 1.0 if key == 'lengths' else 0.0)
      assert (np.abs(stored[ok] - value[ok]) <= 1e-13 * scale).all(), (prefix,
                                                                       key)
  for name, (state, _, _) in results.items():
    same_state(name, state)
  for name, point in points.items():
    same_state(name + '_vec', point['vec'])
    assert abs(float(g[name + '_rate']) - point['rate']) <= (
        1e-12 * point['rate'])
    assert abs(float(g[name + '_psnr_patches']) -
               point['psnr_patches']) <= 1e-9
    assert np.allclose(g[name + '_dequantized'], point['dequantized'],
                       rtol=1e-6, atol=0)
  # the seams the sparse fits cross: two blocks of rows and three rows more,
  # an initial codebook of more than one LDS tile of 23-vectors
  sparse = data.FITS['sparse']
  assert sparse[1] == 2 * data.ROWS + 3 and sparse[2] == 23
  assert data.fit_inputs('sparse')[1].shape[0] > data.tile_codewords(23)
