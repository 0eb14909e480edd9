"""The host half of the baseline JFIF writer (utils/jfif.py) and the numpy
restatement the GPU tests compare the device with (tests/jfif_data.py).

Two links of evidence start here: an outside decoder (PIL, where installed)
opens the restatement's files and agrees with the restatement's own decoder
within the one grey level IEEE 1180 allows an integer IDCT against the float64
one; tests/test_jfif_gpu.py then holds the device to the restatement bit for
bit.  Also: package-merge against brute force, canonical codes, libjpeg's
quality scaling, the scan geometry written out by hand, the header surface.
No GPU needed."""
import ctypes
import heapq
import io
import itertools
import pathlib
import re

import numpy as np
import pytest

import jfif_data as truth

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'ext' / 'vtc_jfif.h'
ENTRY_POINTS = sorted([
    'vtc_jfif_abi_version', 'vtc_jfif_forward_dct', 'vtc_jfif_inverse_dct',
    'vtc_jfif_symbol_counts', 'vtc_jfif_block_bits', 'vtc_jfif_pack',
    'vtc_jfif_stuff_bytes_workspace_bytes', 'vtc_jfif_stuff_bytes'])
COUNT_VALUES = (0, 1, 2, 3, 5, 8, 13, 1000)


def _jfif():
  from utils import jfif
  return jfif


# ------------------------------------------------------ header and bindings
def _code(path):
  return re.sub(r'/\*.*?\*/', '', path.read_text(), flags=re.S)


def test_header_bindings_and_exports():
  import vtc_hip
  declared = {m.group(1): m.group(2) for m in re.finditer(
      r'\b(vtc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', _code(HEADER))}
  assert sorted(declared) == ENTRY_POINTS == sorted(vtc_hip.JFIF_BINDINGS)
  defines = dict(re.findall(r'#define\s+(VTC_[A-Z_]+)\s+(\d+)\b',
                            _code(HEADER)))
  assert {k: int(v) for k, v in defines.items()} == {
      'VTC_JFIF_ABI_VERSION': vtc_hip.JFIF_ABI_VERSION,
      'VTC_JFIF_STUFF_TILE': vtc_hip.JFIF_STUFF_TILE}
  assert 'asm' not in _code(HEADER)
  for name in dir(vtc_hip):
    if name.endswith(('SIGNATURES', '_BINDINGS')) and name != 'JFIF_BINDINGS':
      assert not set(vtc_hip.JFIF_BINDINGS) & set(getattr(vtc_hip, name))
  lib = vtc_hip.load_library()
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declared.items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.JFIF_BINDINGS[name][1]) == count, name
  assert lib.vtc_jfif_abi_version() == vtc_hip.JFIF_ABI_VERSION == 1
  makefile = (REPO / 'vision-transform-codes_amd' / 'csrc' /
              'Makefile').read_text()
  assert 'include/ext/vtc_jfif.h' in makefile
  # the first header stays where it was
  assert lib.vtc_abi_version() == vtc_hip.ABI_VERSION == 4


def test_bad_arguments_are_answered_before_device_work():
  """Host integers as pointers: nothing is dereferenced."""
  import vtc_hip
  lib = vtc_hip.load_library()
  p = [ctypes.c_void_p((i + 1) << 30) for i in range(10)]
  null = ctypes.c_void_p(0)
  INVALID, WORKSPACE = 1, 3

  def refused(rc, status, *words):
    assert rc == status, (rc, lib.vtc_last_error())
    for word in words:
      assert word in lib.vtc_last_error().decode(), lib.vtc_last_error()

  fwd = [p[0], 17, 23, 3, 3, p[1], p[2], p[3], p[4], 9, null]
  for i in (0, 5, 6, 7, 8):
    refused(lib.vtc_jfif_forward_dct(*(fwd[:i] + [null] + fwd[i + 1:])),
            INVALID, 'vtc_jfif_forward_dct', 'null')
  for i, bad in ((1, 0), (2, -1), (3, 2), (4, 2), (9, 0)):
    refused(lib.vtc_jfif_forward_dct(*(fwd[:i] + [bad] + fwd[i + 1:])),
            INVALID, 'vtc_jfif_forward_dct', 'bad size')
  inv = [p[0], 9, p[1], 3, 3, p[2], p[3], p[4], 17, 23, null]
  for i in (0, 2, 5, 6, 7):
    refused(lib.vtc_jfif_inverse_dct(*(inv[:i] + [null] + inv[i + 1:])),
            INVALID, 'vtc_jfif_inverse_dct', 'null')
  refused(lib.vtc_jfif_inverse_dct(*(inv[:3] + [2] + inv[4:])), INVALID,
          'bad size')
  cnt = [p[0], 5, p[1], p[2], p[3], p[4], p[5], null]
  for i in (0, 2, 3, 4, 5, 6):
    refused(lib.vtc_jfif_symbol_counts(*(cnt[:i] + [null] + cnt[i + 1:])),
            INVALID, 'vtc_jfif_symbol_counts', 'null')
  refused(lib.vtc_jfif_symbol_counts(*(cnt[:1] + [0] + cnt[2:])), INVALID,
          'bad size d')
  bits = [p[0], 5, p[1], p[2], p[3], p[4], p[5], p[6], null]
  for i in (0, 2, 3, 4, 5, 6, 7):
    refused(lib.vtc_jfif_block_bits(*(bits[:i] + [null] + bits[i + 1:])),
            INVALID, 'vtc_jfif_block_bits', 'null')
  refused(lib.vtc_jfif_block_bits(*(bits[:1] + [-3] + bits[2:])), INVALID,
          'bad size d')
  pack = [p[0], 5, p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], 100, p[9],
          null]
  for i in (0, 2, 3, 4, 5, 6, 7, 8, 9, 11):
    refused(lib.vtc_jfif_pack(*(pack[:i] + [null] + pack[i + 1:])), INVALID,
            'vtc_jfif_pack', 'null')
  refused(lib.vtc_jfif_pack(*(pack[:10] + [0] + pack[11:])), INVALID,
          'bad size raw_bytes')
  stuff = [p[0], 5000, p[1], 10000, p[2], p[3], p[4], 1 << 20, null]
  assert lib.vtc_jfif_stuff_bytes_workspace_bytes(0) == 0
  assert lib.vtc_jfif_stuff_bytes_workspace_bytes(-4) == 0
  need = lib.vtc_jfif_stuff_bytes_workspace_bytes(5000)
  assert need >= 8 * 3    # one int64 per tile of 2048 bytes
  for i in (0, 2, 4, 5):
    refused(lib.vtc_jfif_stuff_bytes(*(stuff[:i] + [null] + stuff[i + 1:])),
            INVALID, 'vtc_jfif_stuff_bytes', 'null')
  refused(lib.vtc_jfif_stuff_bytes(*(stuff[:1] + [-1] + stuff[2:])), INVALID,
          'bad size n')
  refused(lib.vtc_jfif_stuff_bytes(*(stuff[:3] + [-1] + stuff[4:])), INVALID,
          'bad size capacity')
  refused(lib.vtc_jfif_stuff_bytes(*(stuff[:6] + [null] + stuff[7:])),
          WORKSPACE, 'workspace')
  refused(lib.vtc_jfif_stuff_bytes(*(stuff[:7] + [need - 1] + stuff[8:])),
          WORKSPACE, 'workspace')
  overlap = ctypes.c_void_p(p[0].value + 4999)
  refused(lib.vtc_jfif_stuff_bytes(*(stuff[:2] + [overlap] + stuff[3:])),
          INVALID, 'overlaps')


# ----------------------------------------------------------- package-merge
def _feasible_sorted_lengths(n, limit, reserve):
  """Every non-decreasing length vector of n symbols under `limit` whose
  Kraft sum leaves room for the reserved all-ones leaf of depth `limit`."""
  room = (1 << limit) - (1 if reserve else 0)
  return np.array([v for v in itertools.combinations_with_replacement(
      range(1, limit + 1), n) if sum(1 << (limit - l) for l in v) <= room],
                  dtype=np.int64).reshape(-1, n)


def test_length_limited_lengths_exhaustive_optimality():
  jfif = _jfif()
  feasible = {}
  checked = 0
  for n in range(1, 9):
    for multiset in itertools.combinations_with_replacement(COUNT_VALUES, n):
      used = sorted((c for c in multiset if c), reverse=True)
      for counts in (multiset, multiset[::-1]):
        for limit in (3, 4, 5):
          if len(used) + 1 > 1 << limit:
            with pytest.raises(ValueError):
              jfif.length_limited_lengths(counts, limit)
            continue
          lengths = jfif.length_limited_lengths(counts, limit)
          assert lengths.shape == (n,)
          for c, l in zip(counts, lengths):
            assert (l == 0) == (c == 0) and 0 <= l <= limit
          if not used:
            continue
          kraft = sum(1 << (limit - int(l)) for l in lengths if l)
          assert kraft + 1 <= 1 << limit     # room for the reserved leaf
          key = (len(used), limit)
          if key not in feasible:
            feasible[key] = _feasible_sorted_lengths(len(used), limit, True)
          best = int((feasible[key] * np.array(used, dtype=np.int64)).sum(
              axis=1).min())
          cost = int(sum(int(c) * int(l) for c, l in zip(counts, lengths)))
          assert cost == best, (counts, limit, lengths)
          checked += 1
  assert checked > 50000


def test_length_limited_lengths_without_the_reserved_slot():
  jfif = _jfif()
  for counts, limit in (((5, 5, 5, 5), 2), ((1, 2, 4, 8, 16, 32), 3),
                        ((7,), 4), ((3, 0, 9), 1)):
    lengths = jfif.length_limited_lengths(counts, limit,
                                          reserve_all_ones=False)
    used = sorted((c for c in counts if c), reverse=True)
    table = _feasible_sorted_lengths(len(used), limit, False)
    assert int(sum(c * int(l) for c, l in zip(counts, lengths))) == int(
        (table * np.array(used)).sum(axis=1).min())
  with pytest.raises(ValueError):
    jfif.length_limited_lengths((1, 1, 1), 1, reserve_all_ones=False)
  assert not jfif.length_limited_lengths([0, 0, 0]).any()
  # a function of the counts alone
  a = jfif.length_limited_lengths([4, 4, 4, 4, 4, 1, 1])
  assert np.array_equal(a, jfif.length_limited_lengths([4, 4, 4, 4, 4, 1, 1]))
  assert np.array_equal(a, truth.package_merge([4, 4, 4, 4, 4, 1, 1]))


def _huffman_lengths(counts):
  heap = [(int(c), [s]) for s, c in enumerate(counts) if c > 0]
  lengths = np.zeros(len(counts), dtype=np.int64)
  heapq.heapify(heap)
  while len(heap) > 1:
    a, b = heapq.heappop(heap), heapq.heappop(heap)
    for s in a[1] + b[1]:
      lengths[s] += 1
    heapq.heappush(heap, (a[0] + b[0], a[1] + b[1]))
  return lengths


def test_length_limited_lengths_heavy_tail():
  jfif = _jfif()
  counts = np.array([int(1e12 * 0.9 ** i) + 1 for i in range(256)],
                    dtype=np.int64)
  assert _huffman_lengths(counts).max() > 16
  lengths = jfif.length_limited_lengths(counts)
  assert np.array_equal(lengths, truth.package_merge(counts))
  assert lengths.min() >= 1 and lengths.max() <= 16
  room = (1 << 16) - 1

  def kraft(v):
    return int((1 << (16 - v)).sum())

  assert kraft(lengths) <= room
  codes, bits, huffval = jfif.canonical_codes(lengths)
  for s in range(256):
    assert int(codes[s]) != (1 << int(lengths[s])) - 1, s
  cost = int((counts * lengths).sum())
  rs = np.random.RandomState(16)
  tried = 0
  while tried < 1000:
    other = lengths.copy()
    picks = rs.randint(0, 256, size=rs.randint(2, 7))
    other[picks] += rs.randint(-2, 3, size=len(picks))
    if other.min() < 1 or other.max() > 16 or kraft(other) > room or (
        np.array_equal(other, lengths)):
      continue
    tried += 1
    assert int((counts * other).sum()) >= cost


def test_canonical_codes():
  jfif = _jfif()
  rs = np.random.RandomState(3)
  for trial in range(20):
    counts = rs.randint(0, 50, size=rs.randint(1, 257))
    if not counts.any():
      counts[0] = 1
    lengths = jfif.length_limited_lengths(counts, 16 if trial % 2 else 9)
    codes, bits, huffval = jfif.canonical_codes(lengths)
    used = np.flatnonzero(lengths)
    assert sum(bits) == len(used) == len(huffval) and len(bits) == 16
    assert huffval == sorted(used, key=lambda s: (lengths[s], s))
    words = sorted(format(int(codes[s]), '0%db' % lengths[s]) for s in used)
    for a, b in zip(words, words[1:]):
      assert not b.startswith(a)
    assert all('0' in w for w in words)     # none is all ones
    mine, tbits, tval = truth.canonical(lengths)
    assert (bits, huffval) == (tbits, tval)
    assert all(mine[s] == (int(codes[s]), int(lengths[s])) for s in used)
  with pytest.raises(ValueError):
    jfif.canonical_codes([1, 1, 1])
  with pytest.raises(ValueError):
    jfif.canonical_codes([17])


# ----------------------------------------------------- quantisation tables
def test_quality_tables_are_what_pil_writes():
  Image = pytest.importorskip('PIL.Image')
  jfif = _jfif()
  from utils import jpeg
  picture = Image.fromarray(truth.colour_image(16, 16).astype(np.uint8))
  for quality in (10, 50, 75, 95, 100):
    buf = io.BytesIO()
    picture.save(buf, format='JPEG', quality=quality)
    # the DQT segments as they are in the file: zig-zag order
    written = truth.decode_tables_only(buf.getvalue())
    luma, chroma = jfif.quality_tables(quality)
    assert luma.dtype == chroma.dtype == np.uint16
    assert np.array_equal(luma, written[0]), quality
    assert np.array_equal(chroma, written[1]), quality
    again = truth.quality_tables(quality)
    assert np.array_equal(luma, again[0]) and np.array_equal(chroma, again[1])
    # and PIL's own report of them, in whichever of the two orders it uses
    reported = Image.open(io.BytesIO(buf.getvalue())).quantization
    for mine, theirs in ((luma, reported[0]), (chroma, reported[1])):
      natural = truth.from_zigzag(mine).reshape(-1)
      assert list(theirs) in (mine.tolist(), natural.tolist())
  # Annex K.1 is the table utils.jpeg already holds
  assert np.array_equal(jfif.quality_tables(50)[0],
                        jpeg.get_jpeg_quant_hifi_binwidths())
  assert np.array_equal(jpeg.get_jpeg_quant_hifi_binwidths(),
                        truth.to_zigzag(truth.ANNEX_K1))


def test_quality_tables_arguments():
  jfif = _jfif()
  luma = np.arange(1, 65, dtype=np.uint16)
  chroma = np.full(64, 255, dtype=np.uint16)
  a, b = jfif.quality_tables((luma, chroma))
  assert np.array_equal(a, luma) and np.array_equal(b, chroma)
  a, b = jfif.quality_tables(luma)      # one table for both
  assert np.array_equal(a, luma) and np.array_equal(b, luma)
  for bad in ((luma, np.zeros(64, dtype=np.uint16)),
              (luma[:63], chroma), (luma, chroma.astype(np.int64) + 1),
              (luma.astype(np.float64), chroma)):
    with pytest.raises(ValueError):
      jfif.quality_tables(bad)
  for bad in (0, 101):
    with pytest.raises(ValueError):
      jfif.quality_tables(bad)
  assert jfif.quality_tables(1)[0].max() == 255
  assert (jfif.quality_tables(100)[1] == 1).all()


# ------------------------------------------------------------ scan geometry
def test_scan_layout_33x19_at_420_by_hand():
  jfif = _jfif()
  lay = jfif.scan_layout((33, 19), (2, 2))
  assert lay['rows'] == 36
  assert lay['plane_shapes'] == [(33, 19), (17, 10), (17, 10)]
  assert lay['grids'] == [(6, 4), (3, 2), (3, 2)]
  assert lay['sampling'] == [(2, 2), (1, 1), (1, 1)]
  assert lay['pred'].tolist() == [
      -1, 0, 1, 2, -1, -1,
      3, 6, 7, 8, 4, 5,
      9, 12, 13, 14, 10, 11,
      15, 18, 19, 20, 16, 17,
      21, 24, 25, 26, 22, 23,
      27, 30, 31, 32, 28, 29]
  assert lay['table_sel'].tolist() == [0, 0, 0, 0, 1, 1] * 6
  assert lay['component'].tolist() == [0, 0, 0, 0, 1, 2] * 6
  assert lay['row_of_block'][0].reshape(6, 4).tolist() == [
      [0, 1, 6, 7], [2, 3, 8, 9], [12, 13, 18, 19], [14, 15, 20, 21],
      [24, 25, 30, 31], [26, 27, 32, 33]]
  assert lay['row_of_block'][1].tolist() == [4, 10, 16, 22, 28, 34]
  assert lay['row_of_block'][2].tolist() == [5, 11, 17, 23, 29, 35]
  assert lay['pred'].dtype == np.int32 and lay['table_sel'].dtype == np.uint8


@pytest.mark.parametrize('shape,sub', [((8, 8), None), ((17, 23), None),
                                       ((33, 19), (1, 1)), ((16, 16), (2, 2)),
                                       ((64, 48), (2, 2))])
def test_scan_layout_matches_the_restatement(shape, sub):
  jfif = _jfif()
  lay = jfif.scan_layout(shape, sub)
  rob, pred, sel = truth.scan_arrays(shape, sub)
  assert all(np.array_equal(a, b) for a, b in zip(lay['row_of_block'], rob))
  assert np.array_equal(lay['pred'], pred)
  assert np.array_equal(lay['table_sel'], sel)
  comps, scan = truth.layout(shape, sub)
  assert lay['plane_shapes'] == [c['shape'] for c in comps]
  assert lay['grids'] == [c['grid'] for c in comps]
  assert np.array_equal(jfif.dct_basis(), truth.basis())
  with pytest.raises(NotImplementedError):
    jfif.scan_layout(shape, (2, 1))
  with pytest.raises(ValueError):
    jfif.scan_layout((0, 5), sub)


# ---------------------------------------------------------- the restatement
GRAY = [(8, 8), (16, 16), (17, 23), (64, 48)]
COLOUR = [((16, 16), (1, 1)), ((16, 16), (2, 2)), ((33, 19), (1, 1)),
          ((33, 19), (2, 2))]


def _files():
  """(name, bytes, info, subsampling) of the restatement on the seeded
  inputs."""
  out = []
  for shape in GRAY:
    for quality in (10, 75, 100):
      data, info = truth.encode_gray(truth.gray_image(*shape), quality)
      out.append(('gray-%dx%d-q%d' % (shape + (quality,)), data, info, None))
  data, info = truth.encode_gray(truth.flat_image(17, 23), 75)
  out.append(('flat', data, info, None))
  data, info = truth.encode_gray(truth.noise_image(16, 24), 100)
  out.append(('noise', data, info, None))
  for shape, sub in COLOUR:
    for quality in (10, 75, 100):
      data, info = truth.encode_rgb(truth.colour_image(*shape), sub, quality)
      out.append(('rgb-%dx%d-%d%d-q%d' % (shape + sub + (quality,)), data,
                  info, sub))
  return out


@pytest.fixture(scope='module')
def files():
  return _files()


def test_restatement_round_trip(files):
  for name, data, info, sub in files:
    back = truth.decode(data)
    assert np.array_equal(back['levels'], info['levels']), name
    assert len(back['planes']) == (1 if sub is None else 3)
    for plane, grid, comp in zip(back['planes'], info['grids'],
                                 info['comps']):
      want = truth.inverse_dct(grid, comp['shape'],
                               info['qtables'][comp['tq']])
      assert np.array_equal(plane, want), name
    assert data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9'
    assert data[2:4] == b'\xff\xe0' and data[6:11] == b'JFIF\x00'
    assert info['scan_bits'] == int(info['offsets'][-1])
    assert len(data) == info['header_bytes'] + len(info['raw']) + info[
        'stuffed_bytes']


def test_restatement_edge_streams(files):
  by_name = {name: info for name, _, info, _ in files}
  flat = by_name['flat']
  # every block but the first: DC difference 0 and an end of block
  assert flat['dc_counts'][0, 0] == flat['levels'].shape[0] - 1
  assert flat['ac_counts'][0, 0] == flat['levels'].shape[0]
  assert flat['ac_counts'][0, 1:].sum() == 0
  noise = by_name['noise']
  assert (noise['levels'][:, 63] != 0).all()
  assert noise['ac_counts'][0, 0] == 0          # no end of block at all
  assert noise['stuffed_bytes'] > 0             # 0xFF bytes to stuff
  assert noise['raw'].count(b'\xff') == noise['stuffed_bytes']


def test_pil_opens_the_restatement(files):
  Image = pytest.importorskip('PIL.Image')
  for name, data, info, sub in files:
    mine = truth.decode(data)
    picture = Image.open(io.BytesIO(data))
    assert picture.size == (mine['shape'][1], mine['shape'][0]), name
    if sub is None:
      assert picture.mode == 'L'
      theirs = [np.asarray(picture).astype(np.float64)]
    else:
      picture.draft('YCbCr', picture.size)
      assert picture.mode == 'YCbCr', name
      ycc = np.asarray(picture).astype(np.float64)
      # 4:2:0 chroma passes through PIL's own upsampler: Y only
      theirs = [ycc[..., c] for c in range(3 if sub == (1, 1) else 1)]
    for c, plane in enumerate(theirs):
      worst = np.abs(plane - mine['planes'][c]).max()
      assert worst <= 1.0, '%s plane %d: %g grey levels' % (name, c, worst)


# ------------------------------------------------------- Python-level guards
def test_python_refusals():
  torch = pytest.importorskip('torch')
  import vtc_hip
  jfif = _jfif()
  with pytest.raises(vtc_hip.VtcHipError):
    jfif.encode_gray(torch.zeros(16, 16))
  with pytest.raises(ValueError):
    jfif.encode_gray(torch.zeros(16, 16, 3))
  with pytest.raises(ValueError):
    jfif.encode_rgb(torch.zeros(16, 16))
  with pytest.raises(NotImplementedError):
    jfif.encode_rgb(torch.zeros(16, 16, 3), subsampling=(4, 4))
  with pytest.raises(vtc_hip.VtcHipError):
    jfif.stuff_bytes(torch.zeros(4, dtype=torch.uint8))
  with pytest.raises(vtc_hip.VtcHipError):
    jfif.pack_scan(torch.zeros((1, 64), dtype=torch.int32), [-1], [0],
                   [None, None])
  assert jfif.symbol_of_id(0xF0) == '0:f0'
  assert jfif.symbol_of_id(272 + 256 + 3) == '1:3'
