"""The seventh header, include/vtc_quant.h, held to what
tests/test_code_stats_host.py asks of the sixth: QUANT_SIGNATURES is exactly
the declared surface and shares no name with the other six tables, the library
exports it, the workspace query term for term, bad arguments answered before
any device work; uniform_codebooks and cbook_inds_of_zero_pts against
tests/golden/quantization.npz; the numpy restatement of
tests/quantization_data.py against a brute-force loop; the conditions that keep
the fixture discriminating.  No GPU needed."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import helpers
import quantization_data as data

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'vtc_quant.h'
OTHER_HEADERS = [REPO / 'include' / name
                 for name in ('vtc_hip.h', 'vtc_image.h', 'vtc_codec.h',
                              'vtc_decode.h', 'vtc_quality.h', 'vtc_stats.h')]

OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, 1, 2, 3


def _code(path):
  return re.sub(r'/\*.*?\*/', '', path.read_text(), flags=re.S)


def declarations():
  """name -> argument text of every function include/vtc_quant.h declares."""
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
      'vtc_quant_abi_version', 'vtc_quant_assign', 'vtc_quant_index_counts',
      'vtc_quant_lloyd_step', 'vtc_quant_lloyd_step_workspace_bytes']
  code = _code(HEADER)
  assert re.search(r'#define\s+VTC_QUANT_ABI_VERSION\s+1\b', code)
  assert re.search(r'#define\s+VTC_QUANT_MAX_CODEWORDS\s+1024\b', code)
  assert re.search(r'#define\s+VTC_QUANT_ROWS\s+%d\b' % data.ROWS, code)


def test_the_seven_headers_do_not_overlap():
  for other in OTHER_HEADERS:
    names = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(other)))
    assert names and not names & set(declarations()), other.name


def test_binding_table_is_the_declared_surface():
  vtc_hip, lib = _lib()
  assert sorted(vtc_hip.QUANT_SIGNATURES) == sorted(declarations())
  for other in (vtc_hip.SIGNATURES, vtc_hip.IMAGE_SIGNATURES,
                vtc_hip.CODEC_SIGNATURES, vtc_hip.DECODE_SIGNATURES,
                vtc_hip.QUALITY_SIGNATURES, vtc_hip.STATS_SIGNATURES):
    assert not set(vtc_hip.QUANT_SIGNATURES) & set(other)
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declarations().items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.QUANT_SIGNATURES[name][1]) == count, name
    assert getattr(lib, name).argtypes == vtc_hip.QUANT_SIGNATURES[name][1]
  assert lib.vtc_quant_abi_version() == vtc_hip.QUANT_ABI_VERSION == 1
  assert (vtc_hip.QUANT_MAX_CODEWORDS, vtc_hip.QUANT_ROWS) == (
      data.MAX_CODEWORDS, data.ROWS) == (1024, 512)
  # struct vtc_quant_state: eight pointers in the header's order
  fields = re.search(r'typedef struct vtc_quant_state \{(.*?)\}', _code(HEADER),
                     flags=re.S).group(1)
  assert [f[0] for f in vtc_hip.QuantState._fields_] == re.findall(
      r'\*\s*(\w+)\s*;', fields)
  assert ctypes.sizeof(vtc_hip.QuantState) == 8 * ctypes.sizeof(ctypes.c_void_p)
  # the other six versions stay where they were
  assert lib.vtc_abi_version() == 4
  assert lib.vtc_image_abi_version() == 1
  assert lib.vtc_codec_abi_version() == 1
  assert lib.vtc_decode_abi_version() == 1
  assert lib.vtc_quality_abi_version() == 1
  assert lib.vtc_stats_abi_version() == 1


def test_workspace_query_is_stated_term_for_term():
  _, lib = _lib()
  for b, s, kmax in ((1, 1, 1), (512, 64, 40), (513, 67, 33), (515, 3, 1024),
                     (100000, 64, 41), (1 << 22, 1 << 10, 7)):
    n = -(-b // 512) * s * kmax
    assert lib.vtc_quant_lloyd_step_workspace_bytes(b, s, kmax) == (
        2 * padded(8 * n) + padded(4 * n)), (b, s, kmax)
  for b, s, kmax in ((0, 4, 4), (4, 0, 4), (-1, 4, 4), (4, 4, 0), (4, 4, 1025),
                     (1 << 45, 1 << 20, 4)):
    assert lib.vtc_quant_lloyd_step_workspace_bytes(b, s, kmax) == 0


def _refused(lib, rc, status, *words):
  assert rc == status, (rc, lib.vtc_last_error())
  text = lib.vtc_last_error().decode()
  for word in words:
    assert word in text, text


def _state(vtc_hip, base, skip=None):
  fields = [f[0] for f in vtc_hip.QuantState._fields_]
  return vtc_hip.QuantState(**{name: (0 if name == skip else (base + n) << 20)
                               for n, name in enumerate(fields)})


def test_argument_errors_do_not_touch_the_gpu():
  """Null pointers, bad sizes, unsupported sizes and a short or missing
  workspace, one argument at a time.  The non-null pointers are host integers
  that are never dereferenced: this runs with no device."""
  vtc_hip, lib = _lib()
  p = [ctypes.c_void_p(v << 20) for v in range(1, 12)]

  who = 'vtc_quant_assign'
  #       codes b    s   books lens  k    kmax lam indices deq  status stream
  good = [p[0], 257, 70, p[1], p[2], p[3], 40, 0.5, p[4], p[5], p[6], None]
  for position in (0, 3, 5, 8, 10):
    args = list(good)
    args[position] = None
    _refused(lib, lib.vtc_quant_assign(*args), ERR_INVALID_ARGUMENT, who,
             'null')
  args = list(good)
  args[4] = None   # lengths are needed when lambda != 0
  _refused(lib, lib.vtc_quant_assign(*args), ERR_INVALID_ARGUMENT, who,
           'null', 'lengths')
  for position, value, word in ((1, 0, 'b = 0'), (1, -3, 'b = -3'),
                                (2, 0, 's = 0'), (6, 0, 'kmax = 0'),
                                (7, -1.0, 'lambda'),
                                (7, float('nan'), 'lambda')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_quant_assign(*args), ERR_INVALID_ARGUMENT, who, word)
  args = list(good)
  args[6] = 1025
  _refused(lib, lib.vtc_quant_assign(*args), ERR_UNSUPPORTED, who,
           'kmax = 1025')

  who = 'vtc_quant_lloyd_step'
  need = lib.vtc_quant_lloyd_step_workspace_bytes(257, 70, 40)
  assert need > 0
  state_in, state_out = _state(vtc_hip, 20), _state(vtc_hip, 40)
  #       codes b   s  kmax lam  eps  pin in  out  status ws  bytes stream
  good = [p[0], 257, 70, 40, 0.5, 1e-5, 1, ctypes.byref(state_in),
          ctypes.byref(state_out), p[1], p[2], need, None]
  for position in (0, 7, 8, 9):
    args = list(good)
    args[position] = None
    _refused(lib, lib.vtc_quant_lloyd_step(*args), ERR_INVALID_ARGUMENT, who,
             'null')
  for field, _ in vtc_hip.QuantState._fields_:
    for position, word in ((7, '(in)'), (8, '(out)')):
      args = list(good)
      args[position] = ctypes.byref(_state(vtc_hip, 60, skip=field))
      _refused(lib, lib.vtc_quant_lloyd_step(*args), ERR_INVALID_ARGUMENT,
               who, 'null', word)
  for position, value, word in ((1, 0, 'b = 0'), (2, -1, 's = -1'),
                                (3, 0, 'kmax = 0'), (4, -0.5, 'lambda')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_quant_lloyd_step(*args), ERR_INVALID_ARGUMENT, who,
             word)
  args = list(good)
  args[3] = 1025
  _refused(lib, lib.vtc_quant_lloyd_step(*args), ERR_UNSUPPORTED, who,
           'kmax = 1025')
  args = list(good)
  args[11] = need - 1
  _refused(lib, lib.vtc_quant_lloyd_step(*args), ERR_WORKSPACE, who,
           'workspace', '%d bytes, %d needed' % (need - 1, need))
  args = list(good)
  args[10] = None
  _refused(lib, lib.vtc_quant_lloyd_step(*args), ERR_WORKSPACE, who,
           'workspace')
  # 1024 codewords are supported: this gets as far as the workspace check
  args = list(good)
  args[3], args[11] = 1024, 0
  _refused(lib, lib.vtc_quant_lloyd_step(*args), ERR_WORKSPACE, who,
           'workspace')

  who = 'vtc_quant_index_counts'
  #       indices b   s  kmax counts stream
  good = [p[0], 257, 70, 40, p[1], None]
  for position in (0, 4):
    args = list(good)
    args[position] = None
    _refused(lib, lib.vtc_quant_index_counts(*args), ERR_INVALID_ARGUMENT,
             who, 'null')
  for position, value, word in ((1, 0, 'b = 0'), (2, 0, 's = 0'),
                                (3, -2, 'kmax = -2')):
    args = list(good)
    args[position] = value
    _refused(lib, lib.vtc_quant_index_counts(*args), ERR_INVALID_ARGUMENT,
             who, word)
  args = list(good)
  args[3] = 1025
  _refused(lib, lib.vtc_quant_index_counts(*args), ERR_UNSUPPORTED, who,
           'kmax = 1025')


def test_uniform_codebooks_and_zero_points_match_the_fixture():
  from utils import quantization
  g = helpers.load('quantization')
  books, k = quantization.uniform_codebooks(data.UNIFORM_LO, data.UNIFORM_HI,
                                            data.UNIFORM_W)
  assert books.dtype == np.float64 and k.dtype == np.int32
  assert np.array_equal(k, g['uniform_k'])
  assert np.array_equal(books, g['uniform_codebooks'])   # +inf padding too
  for form in ((books, k), books, {'codebooks': books, 'k': k}):
    zero = quantization.cbook_inds_of_zero_pts(form)
    assert zero.dtype == np.int32
    assert np.array_equal(zero, g['uniform_zero'])
  # ties of rint go to even: 2.5 / 5 -> 0, 7.5 / 5 -> 2
  assert books[2, :3].tolist() == [0.0, 5.0, 10.0] and k[2] == 3
  assert g['uniform_zero'][5] == -1 and g['uniform_zero'][6] == -1
  assert k[7] == 1 and books[7, 0] == 0.0   # NaN range: the zero codeword
  # a codeword past k is not a zero point
  assert quantization.cbook_inds_of_zero_pts(
      (np.array([[1.0, 0.0]]), np.array([1])))[0] == -1
  with pytest.raises(ValueError, match='column 1 needs 1025'):
    quantization.uniform_codebooks([0.0, 0.0], [1.0, 1024.0], [1.0, 1.0])
  quantization.uniform_codebooks([0.0], [1023.0], 1.0)
  with pytest.raises(ValueError):
    quantization.uniform_codebooks([0.0], [1.0], [0.0])


def test_restatement_matches_a_brute_force_loop():
  """Assign and one step of quantization_data on a tiny case against plain
  Python loops."""
  rs = np.random.RandomState(3)
  x = rs.randn(9, 2).astype(np.float32)
  x[::3] = 0.0
  books = np.array([[-1.0, 0.0, 0.75, 9.0], [-0.5, 0.0, 0.5, np.inf]])
  k = np.array([4, 3], np.int32)
  lengths = np.array([[2.0, 1.0, 2.0, 3.0], [1.5, 1.0, 2.5, np.inf]])
  lam = 0.3
  got, _ = data.assign(x, books, k, lengths, lam)
  sums = np.zeros((2, 4))
  members = np.zeros((2, 4), int)
  for r in range(9):
    for j in range(2):
      best, best_i = None, -1
      for i in range(k[j]):
        cost = (float(x[r, j]) - books[j, i]) ** 2 + lam * lengths[j, i]
        if best is None or cost < best:
          best, best_i = cost, i
      assert got[r, j] == best_i
      sums[j, best_i] += float(x[r, j])
      members[j, best_i] += 1
  state = {'codebooks': books, 'lengths': lengths,
           'counts': np.zeros((2, 4), np.int64), 'cost': np.zeros((2, 3)),
           'k': k, 'zero_index': np.array([1, 1], np.int32),
           'active': np.ones(2, np.int32), 'iterations': np.zeros(2, np.int32)}
  new, _ = data.step(x, state, lam, 1e-3, True)
  assert members[0, 3] == 0 and new['k'][0] < 4   # 9.0 has no member
  for j in range(2):
    kept = [i for i in range(k[j]) if members[j, i] or i == 1]
    assert new['k'][j] == len(kept) and new['zero_index'][j] == kept.index(1)
    for p, i in enumerate(kept):
      want = 0.0 if i == 1 else sums[j, i] / members[j, i]
      assert abs(new['codebooks'][j, p] - want) <= 1e-15
      assert new['counts'][j, p] == members[j, i]
    assert (new['codebooks'][j, len(kept):] == 0).all()
  assert (new['iterations'] == 1).all() and (new['active'] == 1).all()


def test_fixture_is_discriminating():
  """What tools/make_quantization_golden.py asserts, asserted again on a fresh
  run of the restatement, and the stored states are that run's: the integers
  equal (the margins keep every assignment and every convergence test away
  from a flip), the float64 fields within 1e-13 relative, since numpy's
  pairwise sums and log2 may differ in the last bits between builds and CPUs
  -- a hundredth of the 1e-11 the GPU tests allow the device."""
  g = helpers.load('quantization')
  results = {name: data.run_fit(name) for name in sorted(data.FITS)}
  facts = data.conditions(results)
  data.check_conditions(facts)
  for key, value in facts.items():
    if isinstance(value, (int, np.integer)):
      assert int(g['fact_' + key]) == value, key
    else:   # ratios of small differences: their own last digits may move
      assert np.isclose(float(g['fact_' + key]), value, rtol=1e-4, atol=0), key
  for name, (state, _, _) in results.items():
    for key, value in state.items():
      stored = g['%s_%s' % (name, key)]
      if key in data.STATE_INT:
        assert np.array_equal(stored, value), (name, key)
        continue
      assert np.array_equal(np.isinf(stored), np.isinf(value)), (name, key)
      assert not np.isnan(stored).any() and not np.isnan(value).any()
      ok = np.isfinite(value)
      scale = np.maximum(np.abs(value[ok]), 1.0 if key == 'lengths' else 0.0)
      assert (np.abs(stored[ok] - value[ok]) <= 1e-13 * scale).all(), (name,
                                                                       key)
  ks = {data.FITS[name][3] for name in data.FITS}
  assert ks == {1, 2, 33, 1024}


def test_cpu_tensors_are_refused():
  import torch
  import vtc_hip
  from utils import quantization
  codes = torch.zeros(8, 2)
  books = (np.zeros((2, 1)), np.ones(2, np.int32))
  with pytest.raises(vtc_hip.VtcHipError):
    quantization.assign(codes, books)
  with pytest.raises(vtc_hip.VtcHipError):
    quantization.scalar_lloyd(codes, books)
  with pytest.raises(vtc_hip.VtcHipError):
    quantization.index_counts(torch.zeros(8, 2, dtype=torch.int32), 4)
  with pytest.raises(vtc_hip.VtcHipError):
    quantization.dequantize_assignments(
        torch.zeros(8, 2, dtype=torch.int32), books)
  with pytest.raises(vtc_hip.VtcHipError):
    quantization.compute_RD_point(codes, torch.zeros(8, 4),
                                  torch.zeros(2, 4), books)
  with pytest.raises(vtc_hip.VtcHipError):
    quantization.Mod1_compute_RD_point(codes, torch.zeros(8, 4),
                                       torch.zeros(2, 4), init_binwidths=1.0)
  with pytest.raises(TypeError):
    quantization.assign(np.zeros((8, 2), np.float32), books)
  assert not hasattr(quantization, 'Mod2_compute_RD_point')
  assert not hasattr(quantization, 'Mod3_compute_RD_point')
