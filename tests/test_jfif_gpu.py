"""The device half of the baseline JFIF writer (csrc/jfif.hip, utils/jfif.py)
against the numpy restatement of tests/jfif_data.py, which
tests/test_jfif_host.py holds to an outside decoder: bytes are compared with
==, levels and planes bit for bit, and every call is run twice and compared.

Whole files on the smallest shapes that take every path (one block, several,
padding on both axes, both subsamplings, a flat image, noise at quality 100);
pack_scan on constructed levels (every zero run around the 16 boundary, every
size of both signs up to the caps, jumping and broken pred chains); stuff_bytes
around the 2048-byte tile; the two DCT calls; the R-D entry point."""
import io

import numpy as np
import pytest
import torch

import jfif_data as truth

pytestmark = pytest.mark.gpu

QUALITIES = (10, 75, 100)


def _jfif():
  from utils import jfif
  return jfif


def _dev(array, device):
  return torch.from_numpy(np.ascontiguousarray(array)).to(device)


def _pil_opens(data, shape):
  try:
    from PIL import Image
  except ImportError:
    return
  picture = Image.open(io.BytesIO(data))
  picture.load()
  assert picture.size == (shape[1], shape[0])


def _same_file(device_result, want, shape):
  (data, info), (want_data, want_info) = device_result, want
  assert np.array_equal(info['levels'].cpu().numpy(), want_info['levels'])
  assert info['scan_bits'] == want_info['scan_bits']
  assert info['stuffed_bytes'] == want_info['stuffed_bytes']
  assert info['header_bytes'] == want_info['header_bytes']
  assert data == want_data
  assert info['file_bytes'] == len(data)
  assert info['bits_per_pixel'] == 8.0 * len(data) / (shape[0] * shape[1])
  _pil_opens(data, shape)


# -------------------------------------------------------------- whole files
GRAY_INPUTS = {
    '8x8': lambda: truth.gray_image(8, 8),
    '16x16': lambda: truth.gray_image(16, 16),
    '17x23': lambda: truth.gray_image(17, 23),
    '64x48': lambda: truth.gray_image(64, 48),
    'flat-17x23': lambda: truth.flat_image(17, 23),
}


@pytest.mark.parametrize('name', sorted(GRAY_INPUTS))
def test_gray_files(device, name):
  jfif = _jfif()
  image = GRAY_INPUTS[name]()
  for quality in QUALITIES:
    want = truth.encode_gray(image, quality)
    first = jfif.encode_gray(_dev(image, device), quality)
    _same_file(first, want, image.shape)
    assert jfif.encode_gray(_dev(image, device), quality)[0] == first[0]
  if name.startswith('flat'):
    # every block: DC difference 0 (but the first) and an end of block
    assert want[1]['ac_counts'][0, 1:].sum() == 0


def test_noise_at_quality_100(device):
  """Q = 1 everywhere: the last coefficient is nonzero, so no block has an
  end of block, the sizes are large and the segment holds 0xFF bytes."""
  jfif = _jfif()
  image = truth.noise_image(16, 24)
  want = truth.encode_gray(image, 100)
  assert want[1]['ac_counts'][0, 0] == 0 and want[1]['stuffed_bytes'] > 0
  first = jfif.encode_gray(_dev(image, device), 100)
  _same_file(first, want, image.shape)
  assert jfif.encode_gray(_dev(image, device), 100)[0] == first[0]


@pytest.mark.parametrize('shape', [(16, 16), (33, 19)])
@pytest.mark.parametrize('sub', [(1, 1), (2, 2)])
def test_colour_files(device, shape, sub):
  jfif = _jfif()
  image = truth.colour_image(*shape)
  for quality in QUALITIES:
    want = truth.encode_rgb(image, sub, quality)
    first = jfif.encode_rgb(_dev(image, device), sub, quality)
    _same_file(first, want, shape)
    assert jfif.encode_rgb(_dev(image, device), sub, quality)[0] == first[0]
    decoded = jfif.decode_levels(first[1]).cpu().numpy()
    back = truth.decode(want[0])
    assert truth.color_data.same_bits(
        decoded, truth.merge_rgb(back['planes'], shape, sub))


def test_caller_supplied_tables_and_write_jpeg(device, tmp_path):
  jfif = _jfif()
  image = truth.gray_image(17, 23)
  luma = (np.arange(64) % 7 + 1).astype(np.uint16)
  chroma = np.full(64, 9, dtype=np.uint16)
  want = truth.encode_gray(image, qtables=(luma, chroma))
  got = jfif.encode_gray(_dev(image, device), qtables=(luma, chroma))
  _same_file(got, want, image.shape)
  path = tmp_path / 'out.jpg'
  info = jfif.write_jpeg(str(path), _dev(image, device),
                         qtables=(luma, chroma))
  assert path.read_bytes() == want[0] and info['file_bytes'] == len(want[0])


# ---------------------------------------------------------------- pack_scan
def _pack_both(device, levels, pred, sel, tables=None):
  """(device raw bytes, device offsets, restatement raw, offsets), the device
  call made twice."""
  jfif = _jfif()
  levels = np.ascontiguousarray(levels, dtype=np.int32)
  tokens = truth.scan_tokens(levels, pred, sel)
  if tables is None:
    tables = truth.build_tables(*truth.count_symbols(tokens))
  want_raw, _, want_offsets = truth.pack_tokens(tokens, tables)
  raw, offsets = jfif.pack_scan(_dev(levels, device), pred, sel, tables)
  again, _ = jfif.pack_scan(_dev(levels, device), pred, sel, tables)
  assert torch.equal(raw, again)
  assert raw.cpu().numpy().tobytes() == want_raw
  assert np.array_equal(offsets.cpu().numpy(), want_offsets)
  ac, dc = jfif.symbol_counts(_dev(levels, device), pred, sel)
  want_ac, want_dc = truth.count_symbols(tokens)
  assert np.array_equal(ac, want_ac) and np.array_equal(dc, want_dc)
  return tables


def _chain(d):
  return np.arange(-1, d - 1, dtype=np.int32)


def test_pack_scan_zero_runs(device):
  rows = []
  for run in (15, 16, 17, 31, 32, 62):
    first = np.zeros(64, dtype=np.int32)     # the run before the first level
    first[0], first[1 + run] = 3, -2
    rows.append(first)
    if run + 3 <= 63:                        # the run between two levels
      between = np.zeros(64, dtype=np.int32)
      between[1], between[2 + run] = 5, 7
      rows.append(between)
      last = np.zeros(64, dtype=np.int32)    # ... ending at index 63
      last[62 - run], last[63] = -1, 1
      rows.append(last)
  only63 = np.zeros(64, dtype=np.int32)
  only63[63] = -9
  rows += [only63, np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int32)]
  dense = np.arange(64, dtype=np.int32) % 5 - 2
  rows.append(dense)
  levels = np.stack(rows)
  d = len(rows)
  assert d % 32 != 0
  _pack_both(device, levels, _chain(d), np.zeros(d, dtype=np.uint8))
  # one row alone
  _pack_both(device, levels[:1], _chain(1), np.zeros(1, dtype=np.uint8))


def test_pack_scan_every_size_of_both_signs(device):
  ac = [2 ** k - 1 for k in range(1, 11)] + [2 ** k for k in range(0, 10)]
  dc = [2 ** k - 1 for k in range(1, 12)] + [2 ** k for k in range(0, 11)]
  rows = []
  for sign in (1, -1):
    for at in range(0, len(ac), 9):
      row = np.zeros(64, dtype=np.int32)
      for j, m in enumerate(ac[at:at + 9]):
        row[1 + 7 * j] = sign * m
      rows.append(row)
  levels = np.stack(rows)
  d = levels.shape[0]
  _pack_both(device, levels, _chain(d), np.zeros(d, dtype=np.uint8))
  # DC differences: every row is predicted from row 0, which holds 0
  levels = np.zeros((1 + 2 * len(dc), 64), dtype=np.int32)
  levels[1:, 0] = [s * m for s in (1, -1) for m in dc]
  pred = np.zeros(levels.shape[0], dtype=np.int32)
  pred[0] = -1
  _pack_both(device, levels, pred, np.zeros(levels.shape[0], dtype=np.uint8))
  # a difference built from two large levels of opposite sign
  levels = np.zeros((2, 64), dtype=np.int32)
  levels[:, 0] = (1000, -1047)
  _pack_both(device, levels, _chain(2), np.zeros(2, dtype=np.uint8))


def test_pack_scan_beyond_the_caps(device):
  jfif = _jfif()
  ok = np.zeros((3, 64), dtype=np.int32)
  ok[:, 0], ok[:, 5] = (1, 2, 3), (1023, -1023, 512)
  sel = np.zeros(3, dtype=np.uint8)
  tables = _pack_both(device, ok, _chain(3), sel)
  for row, index, value in ((1, 5, 1024), (2, 5, -1024), (1, 0, 2050),
                            (2, 0, -2046)):
    bad = ok.copy()
    bad[row, index] = value
    with pytest.raises(ValueError, match='baseline sizes'):
      jfif.pack_scan(_dev(bad, device), _chain(3), sel, tables)
    with pytest.raises(ValueError, match='baseline sizes'):
      jfif.symbol_counts(_dev(bad, device), _chain(3), sel)
    with pytest.raises(ValueError):
      truth.scan_tokens(bad, _chain(3), sel)


def test_pack_scan_pred_chains(device):
  rs = np.random.RandomState(420)
  _, pred, sel = truth.scan_arrays((33, 19), (2, 2))
  d = pred.shape[0]
  levels = (rs.randint(-40, 41, size=(d, 64)) *
            (rs.rand(d, 64) < 0.3)).astype(np.int32)
  levels[:, 0] = rs.randint(-500, 501, size=d)
  _pack_both(device, levels, pred, sel)
  # a chain broken in the middle of the scan, and an entry beyond the rows
  # (read as -1)
  broken = pred.copy()
  broken[[13, 22]] = -1
  _pack_both(device, levels, broken, sel)
  jfif = _jfif()
  tokens = truth.scan_tokens(levels, broken, sel)
  tables = truth.build_tables(*truth.count_symbols(tokens))
  want, _, _ = truth.pack_tokens(tokens, tables)
  beyond = broken.copy()
  beyond[13], beyond[22] = d, -7
  raw, _ = jfif.pack_scan(_dev(levels, device), beyond, sel, tables)
  assert raw.cpu().numpy().tobytes() == want


def test_pack_scan_missing_symbol(device):
  jfif = _jfif()
  levels = np.zeros((2, 64), dtype=np.int32)
  levels[0, 0], levels[0, 3], levels[1, 0] = 4, 1, 4
  sel = np.zeros(2, dtype=np.uint8)
  tables = _pack_both(device, levels, _chain(2), sel)
  other = levels.copy()
  other[1, 20] = 1          # needs ZRL (0xF0) and 0x31, which the tables lack
  with pytest.raises(KeyError) as e:
    jfif.pack_scan(_dev(other, device), _chain(2), sel, tables)
  assert e.value.args[0] == '0:31'
  with pytest.raises(KeyError):
    truth.pack_tokens(truth.scan_tokens(other, _chain(2), sel), tables)
  # the same rows under table pair 1, which was never built
  with pytest.raises(KeyError) as e:
    jfif.pack_scan(_dev(levels, device), _chain(2),
                   np.ones(2, dtype=np.uint8), tables)
  assert e.value.args[0].startswith('1:')


# -------------------------------------------------------------- stuff_bytes
def _stuff_both(device, raw, capacity=None):
  jfif = _jfif()
  raw = np.ascontiguousarray(raw, dtype=np.uint8)
  want = truth.stuff(raw.tobytes())
  out, length, dropped = jfif.stuff_bytes(_dev(raw, device), capacity)
  again = jfif.stuff_bytes(_dev(raw, device), capacity)
  assert torch.equal(out, again[0]) and again[1:] == (length, dropped)
  assert length == len(want)
  room = len(want) if capacity is None else capacity
  assert dropped == max(0, len(want) - room)
  assert out.cpu().numpy().tobytes() == want[:room]


@pytest.mark.parametrize('n', [0, 1, 2047, 2048, 2049, 4097])
def test_stuff_bytes_lengths(device, n):
  rs = np.random.RandomState(n)
  raw = rs.randint(0, 256, size=n).astype(np.uint8)
  raw[rs.rand(n) < 0.2] = 0xFF
  _stuff_both(device, raw)
  _stuff_both(device, np.where(raw == 0xFF, 0xFE, raw))    # 0xFF nowhere
  _stuff_both(device, np.full(n, 0xFF, dtype=np.uint8))    # 0xFF everywhere


def test_stuff_bytes_at_the_tile_boundary(device):
  for marks in ((2047,), (2048,), (2047, 2048), (0, 4096), (2047, 2048, 4095,
                                                           4096)):
    raw = np.arange(4097, dtype=np.int64).astype(np.uint8)
    raw[raw == 0xFF] = 0x11
    raw[list(marks)] = 0xFF
    _stuff_both(device, raw)


def test_stuff_bytes_capacity_one_short(device):
  rs = np.random.RandomState(9)
  raw = rs.randint(0, 256, size=4097).astype(np.uint8)
  raw[rs.rand(4097) < 0.1] = 0xFF
  need = len(truth.stuff(raw.tobytes()))
  _stuff_both(device, raw, need)
  _stuff_both(device, raw, need - 1)
  raw[-1] = 0xFF                # the dropped byte is the inserted zero
  _stuff_both(device, raw, len(truth.stuff(raw.tobytes())) - 1)
  _stuff_both(device, raw, 0)


# ---------------------------------------------------------------------- DCT
@pytest.mark.parametrize('shape,grid', [((8, 8), (1, 1)), ((16, 16), (2, 2)),
                                        ((17, 23), (3, 3)),
                                        ((17, 23), (4, 4)),
                                        ((64, 48), (8, 6))])
def test_dct_and_inverse_bit_equal(device, shape, grid):
  jfif = _jfif()
  image = truth.gray_image(*shape)
  image[0, 0], image[-1, -1] = -3.5, 300.25         # clamped
  if shape[1] > 8:
    image[1, 2:6] = (0.5, 1.5, 2.5, 254.5)          # ties go to even
  blocks = grid[0] * grid[1]
  rob = np.random.RandomState(blocks).permutation(blocks).astype(np.int32)
  for quality in (10, 100):
    q = truth.quality_tables(quality)[0]
    want = truth.forward_dct(image, grid, q).reshape(blocks, 64)
    levels = torch.full((blocks, 64), 12345, dtype=torch.int32, device=device)
    jfif.forward_dct(_dev(image, device), grid, q, rob, levels)
    got = levels.cpu().numpy()
    assert np.array_equal(got[rob], want)
    again = torch.empty_like(levels)
    jfif.forward_dct(_dev(image, device), grid, q, rob, again)
    assert torch.equal(levels, again)
    plane = jfif.inverse_dct(levels, shape, grid, q, rob)
    want_plane = truth.inverse_dct(want.reshape(grid + (64,)), shape, q)
    assert plane.dtype == torch.float32 and tuple(plane.shape) == shape
    assert truth.color_data.same_bits(plane.cpu().numpy(), want_plane)
    assert torch.equal(plane, jfif.inverse_dct(levels, shape, grid, q, rob))


def test_row_of_block_out_of_range(device):
  jfif = _jfif()
  shape, grid = (17, 23), (3, 3)
  image = truth.gray_image(*shape)
  q = truth.quality_tables(75)[0]
  want = truth.forward_dct(image, grid, q).reshape(9, 64)
  rob = np.array([0, -1, 2, 9, 4, 5, -2147483648, 2147483647, 8],
                 dtype=np.int32)
  levels = torch.full((9, 64), 12345, dtype=torch.int32, device=device)
  jfif.forward_dct(_dev(image, device), grid, q, rob, levels)
  got = levels.cpu().numpy()
  for block, row in enumerate(rob):
    if 0 <= row < 9:
      assert np.array_equal(got[row], want[block])
  for row in (1, 3, 6, 7):
    assert (got[row] == 12345).all()
  # the way back reads zeros for such a block: a flat 128
  good = _dev(want.astype(np.int32), device)
  plane = jfif.inverse_dct(good, shape, grid, q, rob).cpu().numpy()
  zeroed = want.copy()
  for block, row in enumerate(rob):
    zeroed[block] = want[row] if 0 <= row < 9 else 0
  assert truth.color_data.same_bits(
      plane, truth.inverse_dct(zeroed.reshape(3, 3, 64), shape, q))
  assert (plane[:8, 8:16] == 128.0).all()


# ---------------------------------------------------------------------- R-D
def test_rate_distortion_image(device):
  jfif = _jfif()
  from utils import plotting
  image = _dev(truth.gray_image(64, 48), device)
  points = []
  for quality in (95, 75, 50, 25):
    r = jfif.rate_distortion_image(image, quality)
    assert list(r)[:4] == ['bits_per_pixel', 'pSNR', 'SSIM', 'tables']
    assert r['bits_per_pixel'] == 8.0 * len(r['bytes']) / (64 * 48)
    decoded = jfif.decode_levels(r['info'])
    assert r['pSNR'] == plotting.compute_pSNR(image, decoded,
                                              manual_sig_mag=255.0)
    assert r['SSIM'] == plotting.compute_ssim(image, decoded,
                                              manual_sig_mag=255.0)
    assert r['bytes'] == truth.encode_gray(image.cpu().numpy(), quality)[0]
    points.append((r['bits_per_pixel'], r['pSNR'], r['SSIM']))
  for (rate, psnr, ssim), (rate2, psnr2, ssim2) in zip(points, points[1:]):
    assert rate2 < rate and psnr2 < psnr and ssim2 < ssim, points
  colour = _dev(truth.colour_image(33, 19), device)
  r = jfif.rate_distortion_image(colour, 75, subsampling=(2, 2))
  decoded = jfif.decode_levels(r['info'])
  assert tuple(decoded.shape) == (33, 19, 3)
  assert r['bits_per_pixel'] == 8.0 * len(r['bytes']) / (33 * 19)
  assert r['pSNR'] == plotting.compute_pSNR(colour, decoded,
                                            manual_sig_mag=255.0)
  ssim = plotting.compute_ssim_images(
      colour.permute(2, 0, 1).contiguous(),
      decoded.permute(2, 0, 1).contiguous(), manual_sig_mag=255.0)
  assert r['SSIM'] == float(ssim.mean())
  assert r['bytes'] == truth.encode_rgb(colour.cpu().numpy(), (2, 2), 75)[0]
