"""The sixth header, include/vtc_stats.h, held to what tests/test_ssim_host.py
asks of the fifth: STATS_SIGNATURES is exactly the declared surface and shares
no name with the other five tables, the library exports it, every workspace
query term for term, bad arguments answered before any device work; the host
arithmetic of utils.plotting (density, kurtosis, joint density) and the host
bin map of utils.misc.rotational_average against tests/golden/code_stats.npz;
the conditions that keep that fixture discriminating.  No GPU needed."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import code_stats_data as data
import helpers

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'vtc_stats.h'
OTHER_HEADERS = [REPO / 'include' / name
                 for name in ('vtc_hip.h', 'vtc_image.h', 'vtc_codec.h',
                              'vtc_decode.h', 'vtc_quality.h')]

OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, 1, 2, 3
F32, F64 = 0, 2
HOST_BOUND = 1e-12


def _code(path):
  return re.sub(r'/\*.*?\*/', '', path.read_text(), flags=re.S)


def declarations():
  """name -> argument text of every function include/vtc_stats.h declares."""
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
      'vtc_binned_mean', 'vtc_binned_mean_workspace_bytes',
      'vtc_code_histogram', 'vtc_code_histogram_workspace_bytes',
      'vtc_code_joint_histogram', 'vtc_code_joint_histogram_workspace_bytes',
      'vtc_code_summary', 'vtc_code_summary_workspace_bytes',
      'vtc_stats_abi_version']
  assert re.search(r'#define\s+VTC_STATS_ABI_VERSION\s+1\b', _code(HEADER))


def test_the_six_headers_do_not_overlap():
  for other in OTHER_HEADERS:
    names = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(other)))
    assert names and not names & set(declarations()), other.name


def test_binding_table_is_the_declared_surface():
  vtc_hip, lib = _lib()
  assert sorted(vtc_hip.STATS_SIGNATURES) == sorted(declarations())
  for other in (vtc_hip.SIGNATURES, vtc_hip.IMAGE_SIGNATURES,
                vtc_hip.CODEC_SIGNATURES, vtc_hip.DECODE_SIGNATURES,
                vtc_hip.QUALITY_SIGNATURES):
    assert not set(vtc_hip.STATS_SIGNATURES) & set(other)
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declarations().items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.STATS_SIGNATURES[name][1]) == count, name
    assert getattr(lib, name).argtypes == vtc_hip.STATS_SIGNATURES[name][1]
  assert lib.vtc_stats_abi_version() == vtc_hip.STATS_ABI_VERSION == 1
  assert (vtc_hip.STATS_MAX_IGNORE, vtc_hip.STATS_MAX_BINS,
          vtc_hip.STATS_MAX_JOINT_BINS) == (8, 4096, 256)
  # the other five versions stay where they were
  assert lib.vtc_abi_version() == 4
  assert lib.vtc_image_abi_version() == 1
  assert lib.vtc_codec_abi_version() == 1
  assert lib.vtc_decode_abi_version() == 1
  assert lib.vtc_quality_abi_version() == 1


def test_workspace_queries_are_stated_term_for_term():
  """Each query against the formula of its header comment; host-only; 0 for a
  shape the call refuses."""
  _, lib = _lib()
  for b, s in ((1, 1), (512, 64), (513, 65), (4099, 70), (131072, 1024),
               (1 << 22, 1 << 10)):
    n = -(-b // 512) * s
    assert lib.vtc_code_summary_workspace_bytes(b, s) == (
        padded(8 * n) + 4 * padded(4 * n)), (b, s)
  for b, s in ((0, 4), (4, 0), (-1, 4)):
    assert lib.vtc_code_summary_workspace_bytes(b, s) == 0

  for b, s, bins in ((1, 1, 1), (4099, 70, 100), (5, 4096, 4096)):
    assert lib.vtc_code_histogram_workspace_bytes(b, s, bins) == (
        2 * padded(8 * s)), (b, s, bins)
  for b, s, bins in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (4, 4, 4097)):
    assert lib.vtc_code_histogram_workspace_bytes(b, s, bins) == 0

  for b, pairs in ((1, 1), (4096, 3), (4099, 3), (131072, 64)):
    n = pairs * -(-b // 4096)
    assert lib.vtc_code_joint_histogram_workspace_bytes(b, pairs) == (
        5 * padded(4 * n)), (b, pairs)
  for b, pairs in ((0, 1), (1, 0)):
    assert lib.vtc_code_joint_histogram_workspace_bytes(b, pairs) == 0

  for count, h, w, nbins in ((1, 1, 1, 1), (3, 17, 33, 6), (2, 64, 65, 300),
                             (5, 256, 256, 4096)):
    c = -(-h * w // 4096)
    assert lib.vtc_binned_mean_workspace_bytes(count, h, w, nbins) == (
        padded(8 * count * c * nbins) + padded(4 * c * nbins)), (count, h, w)
  for count, h, w, nbins in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4),
                             (1, 4, 4, 0), (1, 4, 4, 4097)):
    assert lib.vtc_binned_mean_workspace_bytes(count, h, w, nbins) == 0


def _refused(lib, rc, status, *words):
  assert rc == status, (rc, lib.vtc_last_error())
  text = lib.vtc_last_error().decode()
  for word in words:
    assert word in text, text


def _sweep(lib, fn, who, good, pointers, bad_values, unsupported, ws_at):
  """Null pointers, bad sizes, unsupported sizes and a short or missing
  workspace, one argument at a time.  The non-null pointers are host integers
  that are never dereferenced: this runs with no device."""
  assert ws_at == len(good) - 3
  need = good[ws_at + 1]
  assert need > 0
  for position in pointers:
    args = list(good)
    args[position] = None
    _refused(lib, fn(*args), ERR_INVALID_ARGUMENT, who, 'null')
  for position, value, word in bad_values:
    args = list(good)
    args[position] = value
    _refused(lib, fn(*args), ERR_INVALID_ARGUMENT, who, word)
  for position, value, word in unsupported:
    args = list(good)
    args[position] = value
    _refused(lib, fn(*args), ERR_UNSUPPORTED, who, word)
  args = list(good)
  args[ws_at + 1] = need - 1
  _refused(lib, fn(*args), ERR_WORKSPACE, who, 'workspace',
           '%d bytes, %d needed' % (need - 1, need))
  args = list(good)
  args[ws_at] = None
  _refused(lib, fn(*args), ERR_WORKSPACE, who, 'workspace')


def test_argument_errors_do_not_touch_the_gpu():
  _, lib = _lib()
  p = [ctypes.c_void_p(v << 20) for v in range(1, 12)]

  need = lib.vtc_code_summary_workspace_bytes(257, 70)
  #       codes b   s   ignore n kept lo hi mean var nonf ws bytes stream
  good = [p[0], 257, 70, p[1], 1, p[2], p[3], p[4], p[5], p[6], p[7], p[8],
          need, None]
  _sweep(lib, lib.vtc_code_summary, 'vtc_code_summary', good,
         (0, 3, 5, 6, 7, 8, 9, 10),
         ((1, 0, 'b = 0'), (1, -3, 'b = -3'), (2, 0, 's = 0'),
          (4, 9, 'n_ignore = 9'), (4, -1, 'n_ignore = -1')), (), 11)
  # no list, no pointer needed: this gets as far as the workspace check
  args = list(good)
  args[3], args[4], args[12] = None, 0, 0
  _refused(lib, lib.vtc_code_summary(*args), ERR_WORKSPACE, 'workspace')

  need = lib.vtc_code_histogram_workspace_bytes(257, 70, 7)
  #       codes b   s   ignore n lo   hi  bins counts ws bytes stream
  good = [p[0], 257, 70, p[1], 1, p[2], p[3], 7, p[4], p[5], need, None]
  _sweep(lib, lib.vtc_code_histogram, 'vtc_code_histogram', good,
         (0, 3, 5, 6, 8),
         ((1, 0, 'b = 0'), (2, 0, 's = 0'), (2, -1, 's = -1'),
          (4, 9, 'n_ignore = 9'), (7, 0, 'bins = 0')),
         ((7, 4097, 'bins = 4097'),), 9)
  # 4096 bins are supported: this gets as far as the workspace check
  args = list(good)
  args[7] = 4096
  args[10] = lib.vtc_code_histogram_workspace_bytes(257, 70, 4096) - 1
  _refused(lib, lib.vtc_code_histogram(*args), ERR_WORKSPACE, 'workspace')

  need = lib.vtc_code_joint_histogram_workspace_bytes(257, 3)
  #       codes b   s   pairs P max ignore n bins kept lo hi counts ws bytes
  good = [p[0], 257, 70, p[1], 3, 70, p[2], 1, 16, p[3], p[4], p[5], p[6],
          p[7], need, None]
  _sweep(lib, lib.vtc_code_joint_histogram, 'vtc_code_joint_histogram', good,
         (0, 3, 6, 9, 10, 11, 12),
         ((1, 0, 'b = 0'), (2, 0, 's = 0'), (4, 0, 'n_pairs = 0'),
          (5, 0, 'max_column = 0'), (5, 71, 'max_column = 71'),
          (7, 9, 'n_ignore = 9'), (8, 0, 'bins = 0')),
         ((8, 257, 'bins = 257'),), 13)

  need = lib.vtc_binned_mean_workspace_bytes(3, 17, 33, 6)
  #       images dtype bin_of count h  w  nbins means members ws bytes stream
  good = [p[0], F32, p[1], 3, 17, 33, 6, p[2], p[3], p[4], need, None]
  _sweep(lib, lib.vtc_binned_mean, 'vtc_binned_mean', good, (0, 2, 7, 8),
         ((3, 0, 'count = 0'), (4, 0, 'h = 0'), (5, -1, 'w = -1'),
          (1, 1, 'dtype 1'), (1, 3, 'dtype 3'), (6, 0, 'nbins = 0')),
         ((6, 4097, 'nbins = 4097'),), 9)


def test_fixture_is_discriminating():
  """The three things tools/make_code_stats_golden.py asserts about the
  marginal fixture, asserted again on what is stored."""
  g = helpers.load('code_stats')
  x = data.marginal_codes()
  assert x.shape == (data.ROWS, data.COLS) and x.dtype == np.float32
  assert 0.65 < (x == 0).mean() < 0.75
  lo, hi, kept = g['min_zero'], g['max_zero'], g['kept_zero']
  differs = 0
  for c in range(data.COLS):
    values = data.kept_values(x[:, c], [0.0])
    assert len(values) == kept[c]
    if not len(values) or lo[c] == hi[c]:
      continue
    for bins in data.BINS:
      differs += not np.array_equal(
          data.floor_formula_bins(values, lo[c], hi[c], bins),
          g['counts_zero_%d' % bins][c])
  assert differs == int(g['floor_formula_differs']) >= 1
  assert lo[data.CONSTANT] == hi[data.CONSTANT] == 1.5
  assert lo[data.LAST_ONLY] == hi[data.LAST_ONLY] == -2.25
  assert kept[data.LAST_ONLY] == 1
  assert kept[data.ALL_ZERO] == 0 and np.isnan(lo[data.ALL_ZERO])
  # lo == hi: everything in the LAST bin
  assert g['counts_zero_7'][data.CONSTANT].tolist() == [0] * 6 + [data.ROWS]
  assert g['joint_kept'][-1] == 0 and np.isnan(g['joint_lo'][-1]).all()
  assert g['variance_f32_zero'].dtype == np.float32


def test_host_arithmetic_matches_the_fixture():
  """Density, kurtosis and joint density from given counts, on CPU tensors:
  the same functions code_marginal_densities and code_joint_densities apply to
  the device counts."""
  import torch
  from utils import plotting
  g = helpers.load('code_stats')
  for name in data.VARIANTS:
    counts = torch.from_numpy(g['counts_%s_7' % name].astype(np.int64))
    density = plotting.marginal_density(counts).numpy()
    want = g['density_%s_7' % name]
    assert np.array_equal(np.isnan(density), np.isnan(want))
    assert np.nanmax(np.abs(density - want) / np.maximum(want, 1e-300),
                     initial=0) <= HOST_BOUND
    for bins in data.BINS:
      counts = torch.from_numpy(
          g['counts_%s_%d' % (name, bins)].astype(np.int64))
      got = plotting.pearson_kurtosis(
          plotting.marginal_density(counts)).numpy()
      want = g['kurtosis_%s_%d' % (name, bins)]
      assert np.array_equal(np.isnan(got), np.isnan(want)), (name, bins)
      ok = ~np.isnan(want)
      assert (np.abs(got[ok] - want[ok]) <= HOST_BOUND * want[ok]).all()
  lo, hi = torch.from_numpy(g['joint_lo']), torch.from_numpy(g['joint_hi'])
  kept = torch.from_numpy(g['joint_kept'].astype(np.int64))
  counts = torch.from_numpy(np.stack(
      [g['joint_counts_%d_%d_16' % pair].astype(np.int64)
       for pair in data.PAIRS]))
  x_edges = plotting._linspace_edges(lo[:, 0], hi[:, 0], 16)
  y_edges = plotting._linspace_edges(lo[:, 1], hi[:, 1], 16)
  density = plotting.joint_density(counts, kept, x_edges, y_edges).numpy()
  for n, pair in enumerate(data.PAIRS):
    if not int(kept[n]):
      assert np.isnan(density[n]).all()
      continue
    want = g['joint_density_%d_%d' % pair]
    assert np.array_equal(x_edges[n].numpy(), data.float64_edges(
        g['joint_lo'][n, 0], g['joint_hi'][n, 0], 16))
    assert (np.abs(density[n] - want) <= HOST_BOUND * want).all(), pair


def test_linspace_edges_are_numpy_bit_for_bit():
  import torch
  from utils import plotting
  rs = np.random.RandomState(5)
  lo = rs.randn(200) * 10.0 ** rs.randint(-3, 4, size=200)
  hi = lo + np.abs(rs.randn(200)) * 10.0 ** rs.randint(-3, 4, size=200)
  hi[:5] = lo[:5]
  for bins in (1, 7, 100, 1000):
    got = plotting._linspace_edges(torch.from_numpy(lo), torch.from_numpy(hi),
                                   bins).numpy()
    want = np.stack([np.linspace(a, b, bins + 1) for a, b in zip(lo, hi)])
    assert np.array_equal(got, want), bins


@pytest.mark.parametrize('name', sorted(data.ROTATIONAL))
def test_rotational_bin_map_is_the_reference_assignment(name):
  from utils import misc
  g = helpers.load('code_stats')
  h, w, nbins, _ = data.ROTATIONAL[name]
  _, coords = data.rotational_inputs(name)
  bin_of, edges = misc.rotational_bin_map((h, w), nbins, coords)
  assert bin_of.dtype == np.int32 and bin_of.shape == (h, w)
  assert np.array_equal(bin_of, g['rot_assign_' + name])
  assert np.array_equal(edges, g['rot_edges_' + name])
  members = np.bincount(bin_of.reshape(-1), minlength=nbins + 1)[:nbins]
  assert np.array_equal(members, g['rot_members_' + name])
  assert not bin_of.flags.writeable and not edges.flags.writeable
  if coords is None:   # cached per (shape, nbins), and safe to share
    assert misc.rotational_bin_map((h, w), nbins)[0] is bin_of


def test_error_mapping_of_the_python_layer():
  import torch
  import vtc_hip
  from utils import misc
  from utils import plotting
  codes = torch.zeros(8, 4)
  with pytest.raises(vtc_hip.VtcHipError):
    plotting.code_marginal_densities(codes, 10, [0.0])
  with pytest.raises(vtc_hip.VtcHipError):
    plotting.code_joint_densities(codes, [(0, 1)], 10)
  with pytest.raises(vtc_hip.VtcHipError):
    plotting.code_joint_density(codes[:, :2], 10)
  with pytest.raises(vtc_hip.VtcHipError):
    misc.rotational_average(torch.zeros(16, 16))
  with pytest.raises(ValueError):
    plotting.code_marginal_densities(torch.zeros(8), 10)
  with pytest.raises(ValueError):
    plotting.code_marginal_densities(codes, 0)
  with pytest.raises(ValueError):
    plotting.code_marginal_densities(codes, 4097)
  with pytest.raises(ValueError):
    plotting.code_joint_densities(codes, [(0, 1)], 257)
  with pytest.raises(ValueError):
    plotting.code_marginal_densities(codes, 10, [float(v) for v in range(9)])
  with pytest.raises(TypeError):
    plotting.code_marginal_densities(np.zeros((8, 4), np.float32), 10)
  with pytest.raises(ValueError):
    misc.rotational_average(torch.zeros(4))
  import training.sparse_coding
  assert (misc.load_newest_dictionary_checkpoint is
          training.sparse_coding.load_newest_dictionary_checkpoint)
