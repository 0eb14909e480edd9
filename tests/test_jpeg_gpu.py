"""utils/jpeg.py on the device against tests/golden/jpeg.npz, the reference's
own symbols, tables and streams (tools/make_jpeg_golden.py).  Everything is
integer: every comparison is exact equality.

The fixture is loaded once per module and never written.  Per patch length s
in 1, 2, 17, 18, 63, 64, 65, 130, 300 it holds random rows at densities 0,
0.02, 0.1, 0.5, 1 (v[0] = 0 in a third) and constructed rows: zero runs of 15,
16, 17, 31, 32, 33 (and 255 for s = 300) between two levels, from index 1 and
behind a DC level; runs across a 64-lane chunk boundary and across a whole
chunk; only v[0]; all zero; the last level at s - 1; magnitudes 2^k - 1 and
2^k, k = 0..14, of both signs, as AC and as DC levels.  Batch sizes 1 and 3
(fewer rows than a block has waves), 257 (a ragged last block) and 5000 (every
histogram bin collides).  Every call runs twice and must give equal bytes.
"""
import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 17, 18, 63, 64, 65, 130, 300]


@pytest.fixture(scope='module')
def golden():
  g = helpers.load('jpeg')
  assert g['lengths'].tolist() == LENGTHS
  return {k: g[k] for k in g.files}


def _strings(array):
  return [b.decode('ascii') for b in array.tolist()]


def _tables(golden, tag):
  return tuple(dict(zip(_strings(golden['table_%s_symbols_%s' % (kind, tag)]),
                        _strings(golden['table_%s_codes_%s' % (kind, tag)])))
               for kind in ('ac', 'dc'))


def _same_table(ours, want):
  """String for string, in the reference's order."""
  return list(ours.items()) == list(want.items())


def _dev(array, device):
  return helpers.to_dev(np.ascontiguousarray(array, dtype=np.int32), device)


def _twice(fn):
  """fn() twice; tensors and arrays of the two results must hold equal bytes."""
  first, second = fn(), fn()
  a = first if isinstance(first, tuple) else (first,)
  b = second if isinstance(second, tuple) else (second,)
  for x, y in zip(a, b):
    if torch.is_tensor(x):
      assert x.dtype == y.dtype and torch.equal(x, y)
    else:
      assert np.array_equal(x, y)
  return first


def _bitstring(packed, total):
  bits = np.unpackbits(packed.cpu().numpy())
  assert not bits[total:].any() and bits.size - total < 8
  return ''.join('1' if b else '0' for b in bits[:total])


def check_rows(golden, device, levels, ac, dc, streams, tables,
               tables_are_of_these_rows):
  """Counts, tables, stream lengths, offsets and packed bits of `levels`
  against the reference's symbols `ac` / `dc` and `streams` under `tables`."""
  from utils import jpeg
  lv = _dev(levels, device)
  d = lv.shape[0]
  ac_counts, dc_counts = _twice(lambda: jpeg.symbol_counts(lv))
  assert np.array_equal(ac_counts, np.bincount(ac, minlength=256))
  assert np.array_equal(dc_counts, np.bincount(dc, minlength=16))
  if tables_are_of_these_rows:
    ours = jpeg.tables_from_counts(ac_counts, dc_counts)
    assert _same_table(ours[0], tables[0]) and _same_table(ours[1], tables[1])
  bits = _twice(lambda: jpeg.stream_bits(lv, *tables))
  lengths = np.array([len(x) for x in streams], dtype=np.int64)
  assert bits.dtype == torch.int32
  assert np.array_equal(bits.cpu().numpy(), lengths)
  offsets = _twice(lambda: jpeg.bit_offsets(bits))
  want_offsets = np.concatenate([[0], np.cumsum(lengths)])
  assert offsets.dtype == torch.int64
  assert np.array_equal(offsets.cpu().numpy(), want_offsets)
  packed, pack_offsets = _twice(lambda: jpeg.pack_streams(lv, *tables))
  assert packed.dtype == torch.uint8
  assert np.array_equal(pack_offsets.cpu().numpy(), want_offsets)
  assert _bitstring(packed, int(want_offsets[-1])) == ''.join(streams)
  for i in sorted(set([0, d // 2, d - 1])):
    assert jpeg.stream_as_str(packed, pack_offsets, i) == streams[i]


def _case(golden, tag, rows=None):
  levels = golden['levels_' + tag].astype(np.int32)
  ac_rows = golden['ac_rows_' + tag]
  rows = list(range(len(levels))) if rows is None else rows
  ac = np.concatenate([golden['ac_' + tag][ac_rows[i]:ac_rows[i + 1]]
                       for i in rows])
  streams = _strings(golden['streams_' + tag])
  return (levels[rows], ac, golden['dc_' + tag][rows],
          [streams[i] for i in rows])


@pytest.mark.parametrize('s', LENGTHS)
def test_every_patch_length(golden, device, s):
  levels, ac, dc, streams = _case(golden, str(s))
  assert levels.shape[1] == s and (levels[:, 0] == 0).any()
  check_rows(golden, device, levels, ac, dc, streams, _tables(golden, str(s)),
             True)


@pytest.mark.parametrize('d', [1, 3])
def test_fewer_rows_than_waves(golden, device, d):
  dense = int(np.argmax((golden['levels_64'] != 0).sum(1)))
  rows = [dense, 13, 2][:d]
  levels, ac, dc, streams = _case(golden, '64', rows)
  check_rows(golden, device, levels, ac, dc, streams, _tables(golden, '64'),
             False)


def test_257_rows_of_64(golden, device):
  levels, ac, dc, streams = _case(golden, 'b257')
  assert levels.shape == (257, 64)
  check_rows(golden, device, levels, ac, dc, streams, _tables(golden, 'b257'),
             True)


def test_5_rows_of_130(golden, device):
  l130 = golden['levels_130']
  rows = [int(np.argmax((l130 != 0).sum(1))), 14]
  rows += [i for i, r in enumerate(l130)
           if np.count_nonzero(r) == 2 and ((r[3] and r[129]) or
                                            (r[60] and r[70]) or
                                            (r[63] and r[64]))]
  assert len(rows) == 5
  levels, ac, dc, streams = _case(golden, '130', rows)
  check_rows(golden, device, levels, ac, dc, streams, _tables(golden, '130'),
             False)


def test_5000_rows_of_64(golden, device):
  """Every histogram bin of a block is hit from many waves, and the flush
  from 20 blocks; the offsets run over three tiles."""
  from utils import jpeg
  lv = _dev(golden['levels_b5000'], device)
  assert lv.shape == (5000, 64)
  ac_counts, dc_counts = _twice(lambda: jpeg.symbol_counts(lv))
  assert np.array_equal(ac_counts, golden['counts_ac_b5000'])
  assert np.array_equal(dc_counts, golden['counts_dc_b5000'])
  tables = jpeg.tables_from_counts(ac_counts, dc_counts)
  want = _tables(golden, 'b5000')
  assert _same_table(tables[0], want[0]) and _same_table(tables[1], want[1])
  bits = _twice(lambda: jpeg.stream_bits(lv, *tables))
  assert np.array_equal(bits.cpu().numpy(), golden['bits_b5000'])
  offsets = _twice(lambda: jpeg.bit_offsets(bits))
  assert np.array_equal(
      offsets.cpu().numpy(),
      np.concatenate([[0], np.cumsum(golden['bits_b5000'].astype(np.int64))]))
  packed, pack_offsets = _twice(lambda: jpeg.pack_streams(lv, *tables))
  assert torch.equal(pack_offsets, offsets)
  assert packed.numel() == -(-int(offsets[-1]) // 8)


def test_the_references_interface(golden, device):
  """generate_ac_dc_huffman_tables and generate_jpg_binary_stream with the
  reference's arguments: codeword indices and the index of the zero codeword
  in each dimension."""
  from utils import jpeg
  levels, _, _, _ = _case(golden, 'b257')
  zero = (np.arange(64) % 7 + 300).astype(np.int64)
  inds = torch.from_numpy(levels.astype(np.int64) + zero).to(device)
  assert int(inds.min()) >= 0
  table_ac, table_dc = jpeg.generate_ac_dc_huffman_tables(inds, zero)
  want = _tables(golden, 'b257')
  assert _same_table(table_ac, want[0]) and _same_table(table_dc, want[1])

  for tag, rows in (('64', [25, 31, 40]), ('130', [25, 50]), ('1', [3, 40]),
                    ('300', [28, 45])):
    levels, _, _, streams = _case(golden, tag, rows)
    tables = _tables(golden, tag)
    s = levels.shape[1]
    zero = (np.arange(s) % 5 + 40000).astype(np.int64)
    for i, row in enumerate(rows):
      one = torch.from_numpy(levels[i].astype(np.int64) + zero).to(device)
      first = golden['ac_rows_' + tag][row]
      last = golden['ac_rows_' + tag][row + 1]
      want_ac = ['%x%x' % (b >> 4, b & 15)
                 for b in golden['ac_' + tag][first:last].tolist()]
      category = int(golden['dc_' + tag][row])
      got = jpeg.generate_jpg_binary_stream(one, zero)
      assert isinstance(got, tuple) and isinstance(got[0], list)
      assert got == (want_ac, '-' if category == 0 else '%x' % category)
      stream = jpeg.generate_jpg_binary_stream(one, zero, False, *tables)
      assert isinstance(stream, str) and stream == streams[i]


# ------------------------------------------------------------------ quantise
def test_quantize_is_numpy_rint_in_float64(device):
  from utils import jpeg, matrix_zigzag
  rs = np.random.RandomState(8)
  widths = jpeg.get_jpeg_quant_hifi_binwidths()
  codes = rs.laplace(scale=60, size=(257, 64)).astype(np.float32)
  # exact ties at width 16 (scan position 0 and, under the zig-zag order,
  # coefficient 0 again), and at every width: (k + 0.5) * width is exact in
  # float32 for these integer widths
  codes[0, :4] = [8, 24, -8, -24]
  codes[1:5, 0] = [8, 24, -8, -24]
  codes[5] = (widths * 2.5).astype(np.float32)
  codes[6] = (widths * -3.5).astype(np.float32)
  codes[7, :4] = [np.nan, np.inf, -np.inf, 3e12]
  x = helpers.to_dev(codes, device)
  with np.errstate(invalid='ignore'):
    want = np.rint(codes.astype(np.float64) / widths)
  got = _twice(lambda: jpeg.quantize(x, widths)).cpu().numpy()
  finite = np.isfinite(want) & (np.abs(want) < 2 ** 31)
  assert np.array_equal(got[finite], want[finite].astype(np.int32))
  assert got[0, 0] == 0 and got[2, 0] == 2 and got[3, 0] == 0
  assert got[4, 0] == -2 and (got[5] == 2).all() and (got[6] == -4).all()
  assert got[7, :4].tolist() == [-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1]

  order = matrix_zigzag.scan_order(8, 8)
  codes[7, :4] = 0
  x = helpers.to_dev(codes, device)
  want = np.rint(codes.astype(np.float64)[:, order] / widths).astype(np.int32)
  got = _twice(lambda: jpeg.quantize(x, widths, order))
  assert np.array_equal(got.cpu().numpy(), want)

  # back: one rounding of the float64 product, and within half a bin of x
  back = _twice(lambda: jpeg.dequantize(got, widths, order)).cpu().numpy()
  exact = np.empty((257, 64))
  exact[:, order] = want.astype(np.float64) * widths
  assert np.array_equal(back, exact.astype(np.float32))
  half = np.empty(64)
  half[order] = widths / 2
  assert (np.abs(back.astype(np.float64) - codes) <= half).all()
  plain = jpeg.dequantize(jpeg.quantize(x, widths), widths).cpu().numpy()
  assert (np.abs(plain.astype(np.float64) - codes) <= widths / 2).all()


# -------------------------------------------------------------------- errors
def test_a_level_of_32768_is_a_value_error(golden, device):
  from utils import jpeg
  tables = _tables(golden, '64')
  levels = golden['levels_64'][:5].astype(np.int32).copy()
  levels[3, 9] = 32767
  jpeg.symbol_counts(_dev(levels, device))
  for value in (32768, -32768, -2 ** 31):
    levels[3, 9] = value
    lv = _dev(levels, device)
    for call in (lambda: jpeg.symbol_counts(lv),
                 lambda: jpeg.stream_bits(lv, *tables),
                 lambda: jpeg.pack_streams(lv, *tables)):
      with pytest.raises(ValueError):
        call()


def test_a_symbol_the_tables_lack_is_a_key_error(golden, device):
  """Tables trained without a zero DC level, then a row with v[0] = 0: the
  reference's dict lookup raises KeyError('-')."""
  from utils import jpeg
  levels = golden['levels_64'].astype(np.int32).copy()
  levels[:, 0] = np.where(levels[:, 0] == 0, 5, levels[:, 0])
  tables = jpeg.tables_from_counts(*jpeg.symbol_counts(_dev(levels, device)))
  assert '-' not in tables[1]
  jpeg.stream_bits(_dev(levels, device), *tables)
  levels[2, 0] = 0
  lv = _dev(levels, device)
  for call in (lambda: jpeg.stream_bits(lv, *tables),
               lambda: jpeg.pack_streams(lv, *tables)):
    with pytest.raises(KeyError) as caught:
      call()
    assert caught.value.args == ('-',)
  # the smallest id wins: an AC symbol (ids 0..255) before any DC category
  ac = dict(tables[0])
  del ac['f0'], ac['01']
  with pytest.raises(KeyError) as caught:
    jpeg.stream_bits(_dev(golden['levels_300'], device), ac, tables[1])
  assert caught.value.args == ('01',)


# --------------------------------------------------------- rate / distortion
def test_rate_distortion_point(golden, device):
  from analysis_transforms.fully_connected import invertible_linear
  from utils import jpeg, plotting
  patches = helpers.to_dev(golden['rd_patches'], device)
  dictionary = helpers.to_dev(golden['rd_dictionary'], device)
  assert patches.shape == (512, 64)
  widths = golden['binwidths']
  order = golden['rd_order']
  rates = []
  for n, multiplier in enumerate(golden['rd_multipliers'].tolist()):
    bpp, psnr, tables = jpeg.rate_distortion_point(
        patches, dictionary, widths, multiplier, order=order)
    want_tables = _tables(golden, 'rd%d' % n)
    assert _same_table(tables[0], want_tables[0])
    assert _same_table(tables[1], want_tables[1])
    assert bpp == int(golden['rd_total_bits_%d' % n]) / (512 * 64.)
    # the composition by hand
    codes = invertible_linear.run(patches, dictionary)
    levels = jpeg.quantize(codes, widths * multiplier, order)
    assert np.array_equal(levels.cpu().numpy(),
                          golden['rd_levels_%d' % n].astype(np.int32))
    back = invertible_linear.apply_filter(
        jpeg.dequantize(levels, widths * multiplier, order), dictionary)
    assert psnr == plotting.compute_pSNR(patches, back)
    assert 20 < psnr < 80
    # tables handed in are used as they are
    again = jpeg.rate_distortion_point(patches, dictionary, widths,
                                       multiplier, tables=tables, order=order)
    assert again[0] == bpp and again[1] == psnr and again[2] is tables
    rates.append((bpp, psnr))
  assert rates[1][0] < rates[0][0] and rates[1][1] < rates[0][1]
