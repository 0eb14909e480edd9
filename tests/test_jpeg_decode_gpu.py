"""The decoder of the packed JPEG streams (include/vtc_decode.h, utils/jpeg.py
unpack_streams / parse_jpg_binary_stream / decode_patches) on the device.

The reference has no decoder, so the truth is what it encodes: the streams,
tables and levels of tests/golden/jpeg.npz (tools/make_jpeg_golden.py), and
round trips through this project's packer, which tests/test_jpeg_gpu.py holds
to the reference bit for bit.  Everything is integer: every comparison is
exact equality, and every call runs twice and must give equal bytes.

Malformed inputs are bounds-checked paths, not faults: `packed` and `levels`
sit inside tests/fences.py guards there and the guards must be intact.

LUT_BITS restates kLutBits of csrc/jpeg_decode.hip: codewords of up to that
many bits are found in the first-level lookup, longer ones by search.
"""
import numpy as np
import pytest
import torch

import fences
import helpers

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 17, 18, 63, 64, 65, 130, 300]
LUT_BITS = 10
OK = 0


def load_golden():
  g = helpers.load('jpeg')
  assert g['lengths'].tolist() == LENGTHS
  return {k: g[k] for k in g.files}


@pytest.fixture(scope='module')
def golden():
  return load_golden()


def _strings(array):
  return [b.decode('ascii') for b in array.tolist()]


def _tables(golden, tag):
  return tuple(dict(zip(_strings(golden['table_%s_symbols_%s' % (kind, tag)]),
                        _strings(golden['table_%s_codes_%s' % (kind, tag)])))
               for kind in ('ac', 'dc'))


def pack_strings(streams, lead=0):
  """(bytes uint8, offsets int64) of the strings back to back behind `lead`
  bits that belong to no row (ones: a reader that starts early sees them)."""
  bits = np.frombuffer(('1' * lead + ''.join(streams)).encode('ascii'),
                       dtype=np.uint8) - ord('0')
  packed = np.packbits(bits) if bits.size else np.zeros(1, dtype=np.uint8)
  offsets = lead + np.concatenate(
      [[0], np.cumsum([len(x) for x in streams])]).astype(np.int64)
  return packed, offsets


def _twice(fn):
  first, second = fn(), fn()
  assert first.dtype == second.dtype and torch.equal(first, second)
  return first


def unpack(device, packed, offsets, s, tables):
  """jpeg.unpack_streams of host arrays, twice; the levels as numpy."""
  from utils import jpeg
  p, o = helpers.to_dev(packed, device), helpers.to_dev(offsets, device)
  levels = _twice(lambda: jpeg.unpack_streams(p, o, s, *tables))
  assert levels.dtype == torch.int32
  assert tuple(levels.shape) == (len(offsets) - 1, s)
  return levels.cpu().numpy()


def fenced_unpack(device, packed, packed_bytes, offsets, s, tables):
  """The raw vtc_jpeg_unpack with `packed` (exactly packed_bytes bytes of it),
  `levels` and `status` inside guard bands, levels and status 0xFF-filled and
  the workspace of exactly the queried size.  Twice; returns (levels, status)
  as numpy once every guard is intact and `packed` is unchanged."""
  import vtc_hip
  from utils import jpeg
  lib = vtc_hip.load_library()
  d = len(offsets) - 1
  dev = jpeg._DeviceTables(tables[0], tables[1], device)
  off = helpers.to_dev(np.asarray(offsets, dtype=np.int64), device)
  results = []
  for _ in range(2):
    source = np.ascontiguousarray(packed[:packed_bytes])
    p, fp = fences.fenced_copy(source, device)
    levels, fl = fences.fenced((d, s), torch.int32, device)
    status, fs = fences.fenced((3,), torch.int64, device)
    need = lib.vtc_jpeg_unpack_workspace_bytes()
    ws, fw = fences.fenced_workspace(need, device)
    rc = lib.vtc_jpeg_unpack(
        vtc_hip.ptr(p), packed_bytes, vtc_hip.ptr(off), d, s,
        vtc_hip.ptr(dev.ac_code), vtc_hip.ptr(dev.ac_len),
        vtc_hip.ptr(dev.dc_code), vtc_hip.ptr(dev.dc_len),
        vtc_hip.ptr(levels), vtc_hip.ptr(status), vtc_hip.ptr(ws), need,
        vtc_hip.current_stream(device))
    torch.cuda.synchronize(device)
    assert rc == OK, lib.vtc_last_error()
    for name, fence in (('packed', fp), ('levels', fl), ('status', fs),
                        ('workspace', fw)):
      fence.assert_intact('vtc_jpeg_unpack: ' + name)
    assert np.array_equal(p.cpu().numpy(), source)
    results.append((levels.cpu().numpy(), status.cpu().numpy()))
  assert np.array_equal(results[0][0], results[1][0])
  assert np.array_equal(results[0][1], results[1][1])
  return results[0][0], results[0][1].tolist()


def expect_malformed(device, packed, packed_bytes, offsets, s, tables, want,
                     count, first):
  """The raw call behind fences reports `count` malformed rows, the first
  being `first`, and gives the levels `want`; unpack_streams raises the
  ValueError that names both."""
  from utils import jpeg
  levels, status = fenced_unpack(device, packed, packed_bytes, offsets, s,
                                 tables)
  assert status == [count, first + 1, 0], status
  assert np.array_equal(levels[:first], want[:first])
  assert np.array_equal(levels, want)
  p = helpers.to_dev(np.ascontiguousarray(packed[:packed_bytes]), device)
  o = helpers.to_dev(np.asarray(offsets, dtype=np.int64), device)
  with pytest.raises(ValueError) as caught:
    jpeg.unpack_streams(p, o, s, *tables)
  text = str(caught.value)
  assert '%d malformed rows' % count in text, text
  assert 'the first is row %d' % first in text, text


# ------------------------------------------------------- the reference's bits
@pytest.mark.parametrize('lead', [0, 3, 29])
@pytest.mark.parametrize('tag', [str(s) for s in LENGTHS] + ['b257'])
def test_reference_streams_decode_to_the_reference_levels(golden, device, tag,
                                                          lead):
  """Rows start at every bit phase and across 4-byte words."""
  levels = golden['levels_' + tag].astype(np.int32)
  streams = _strings(golden['streams_' + tag])
  assert len(streams) == levels.shape[0]
  packed, offsets = pack_strings(streams, lead)
  if tag == 'b257':
    assert sorted(set((offsets[:-1] % 8).tolist())) == list(range(8))
  got = unpack(device, packed, offsets, levels.shape[1], _tables(golden, tag))
  assert np.array_equal(got, levels)


@pytest.mark.parametrize('d', [1, 63, 64, 65, 255, 256, 257])
def test_lane_wave_and_block_edges(golden, device, d):
  levels = golden['levels_64'].astype(np.int32)
  streams = _strings(golden['streams_64'])
  rows = [(7 * i) % len(streams) for i in range(d)]
  packed, offsets = pack_strings([streams[i] for i in rows], 5)
  got = unpack(device, packed, offsets, 64, _tables(golden, '64'))
  assert np.array_equal(got, levels[rows])


# ------------------------------------------------ round trips through pack
def _round_trip(device, levels, tables):
  from utils import jpeg
  lv = helpers.to_dev(np.ascontiguousarray(levels, dtype=np.int32), device)
  packed, offsets = jpeg.pack_streams(lv, *tables)
  back = _twice(lambda: jpeg.unpack_streams(packed, offsets, lv.shape[1],
                                            *tables))
  assert torch.equal(back, lv)
  return packed, offsets


def test_round_trip_of_5000_rows(golden, device):
  _round_trip(device, golden['levels_b5000'], _tables(golden, 'b5000'))


def rows_of_4096():
  """Five rows: runs of 15, 16, 17 and 255 zeros; a run of over 4000 zeros; a
  level at index 4095; an all-zero row; every magnitude 2^k - 1 and 2^k of
  both signs up to 32767."""
  magnitudes = sorted(set([(1 << k) - 1 for k in range(1, 16)] +
                          [1 << k for k in range(15)]))
  assert magnitudes[0] == 1 and magnitudes[-1] == 32767
  levels = np.zeros((5, 4096), dtype=np.int32)
  at = 1
  for n, gap in enumerate((15, 16, 17, 255, 0, 31, 32, 33)):
    at += gap
    levels[0, at] = (-1) ** n * (n + 2)
    at += 1
  levels[0, 0] = -7
  levels[1, 0], levels[1, 3], levels[1, 4050] = 1000, -1, 5
  levels[2, 4095] = -32767
  signed = [m for v in magnitudes for m in (v, -v)]
  levels[4, 0] = -32767
  levels[4, 1:1 + len(signed)] = signed
  levels[4, 100:100 + len(signed)] = signed[::-1]
  return levels


def test_round_trip_of_4096_columns(device):
  from utils import jpeg
  levels = rows_of_4096()
  assert not levels[3].any() and levels[2, 4095] and levels[1, 4050]
  lv = helpers.to_dev(levels, device)
  tables = jpeg.tables_from_counts(*jpeg.symbol_counts(lv))
  assert 'f0' in tables[0]
  _round_trip(device, levels, tables)


def unary(i):
  """Codeword i of the code 0, 10, 110, ...: i + 1 bits."""
  return '1' * i + '0'


def skewed_tables(ac_used, dc_used):
  """Prefix-free tables with one codeword of every length 1..64 (AC) and
  1..16 (DC).  The first three AC symbols in use get exactly LUT_BITS,
  LUT_BITS + 1 and 64 bits: the last first-level hit, the first search and
  the longest codeword there is."""
  from utils import jpeg
  assert 3 <= len(ac_used) <= 64
  special = [LUT_BITS, LUT_BITS + 1, 64]
  others = [n for n in range(1, 65) if n not in special]
  spare = [jpeg.ac_symbol(b) for b in range(256)
           if jpeg.ac_symbol(b) not in ac_used]
  symbols = list(ac_used) + spare
  table_ac = {}
  for symbol, bits in zip(symbols, special + others):
    table_ac[symbol] = unary(bits - 1)
  assert sorted(len(w) for w in table_ac.values()) == list(range(1, 65))
  symbols = list(dc_used) + [jpeg.dc_symbol(c) for c in range(16)
                             if jpeg.dc_symbol(c) not in dc_used]
  table_dc = {symbol: unary(i) for i, symbol in enumerate(symbols)}
  return table_ac, table_dc


def test_round_trip_under_codewords_of_1_to_64_bits(device):
  from utils import jpeg
  rs = np.random.RandomState(64)
  levels = (rs.randint(-3, 4, size=(70, 40)) *
            (rs.rand(70, 40) < 0.2)).astype(np.int32)
  levels[:, 0] = rs.randint(-40, 41, size=70)
  ac_counts, dc_counts = jpeg.symbol_counts(helpers.to_dev(levels, device))
  order = np.argsort(-ac_counts, kind='stable')
  ac_used = [jpeg.ac_symbol(b) for b in order.tolist() if ac_counts[b]]
  dc_used = [jpeg.dc_symbol(c) for c in range(16) if dc_counts[c]]
  tables = skewed_tables(ac_used, dc_used)
  for symbol, bits in zip(ac_used, (LUT_BITS, LUT_BITS + 1, 64)):
    assert len(tables[0][symbol]) == bits
  _round_trip(device, levels, tables)
  # and with the lengths handed out the other way round: the rare symbols
  # short, the frequent ones long
  tables = skewed_tables(ac_used[::-1], dc_used[::-1])
  _round_trip(device, levels, tables)


# ------------------------------------------------------------ malformed rows
def _rows_64(golden):
  return (golden['levels_64'].astype(np.int32),
          _strings(golden['streams_64']), _tables(golden, '64'))


def test_a_value_at_index_s_is_malformed(golden, device):
  """Packed with s + 1 columns, unpacked with s: the level in the extra
  column lands at index s.  Its row keeps the AC levels before it; the DC
  part comes after the fault."""
  from utils import jpeg
  levels, _, tables = _rows_64(golden)
  d, s = levels.shape
  wide = np.concatenate([levels, np.zeros((d, 1), dtype=np.int32)], axis=1)
  # a row in the middle with a DC level and its last AC level close enough to
  # the end for the extra token to be a symbol the tables hold (run below 15)
  bad = [i for i in range(1, d - 1)
         if levels[i, 0] and levels[i, s - 14:].any()][0]
  wide[bad, s] = 1
  packed, offsets = jpeg.pack_streams(helpers.to_dev(wide, device), *tables)
  want = levels.copy()
  want[bad, 0] = 0
  expect_malformed(device, packed.cpu().numpy(), packed.numel(),
                   offsets.cpu().numpy(), s, tables, want, 1, bad)


def test_a_stream_cut_by_one_bit_is_malformed(golden, device):
  levels, streams, tables = _rows_64(golden)
  last = int(np.flatnonzero(levels[:, 0])[-1])   # ends in a DC value bit
  rows = [i for i in range(len(streams)) if i != last] + [last]
  levels, streams = levels[rows], [streams[i] for i in rows]
  packed, offsets = pack_strings(streams, 3)
  offsets[-1] -= 1
  want = levels.copy()
  want[-1, 0] = 0
  expect_malformed(device, packed, len(packed), offsets, 64, tables, want, 1,
                   len(streams) - 1)


def test_a_buffer_one_byte_short_is_malformed(golden, device):
  """Every row that ends in the missing byte is malformed, no other."""
  levels, streams, tables = _rows_64(golden)
  packed, offsets = pack_strings(streams, 3)
  limit = 8 * (len(packed) - 1)
  lost = np.flatnonzero(offsets[1:] > limit)
  assert 1 <= len(lost) < len(streams)
  first = int(lost[0])
  got, status = fenced_unpack(device, packed, len(packed) - 1, offsets, 64,
                              tables)
  assert status == [len(lost), first + 1, 0]
  assert np.array_equal(got[:first], levels[:first])
  # of a lost row only levels that are the reference's can have been stored
  assert ((got[first:] == 0) | (got[first:] == levels[first:])).all()
  want = levels.copy()
  want[first:] = got[first:]
  expect_malformed(device, packed, len(packed) - 1, offsets, 64, tables, want,
                   len(lost), first)


def test_a_size_0_byte_of_run_3_is_malformed(golden, device):
  """0x30 is in the padded tables (every run 0..14 with size 0) and means
  nothing: only 0x00 and 0xF0 have size 0."""
  levels, streams, tables = _rows_64(golden)
  assert '30' in tables[0]
  bad = 20
  streams = list(streams)
  keep = tables[0]['01'] + '1'       # one good token first: v[1] = 1
  streams[bad] = keep + tables[0]['30'] + tables[0]['00'] + tables[1]['-']
  packed, offsets = pack_strings(streams, 6)
  want = levels.copy()
  want[bad] = 0
  want[bad, 1] = 1
  expect_malformed(device, packed, len(packed), offsets, 64, tables, want, 1,
                   bad)


def test_a_window_no_codeword_matches_is_malformed(golden, device):
  """A symbol that one row alone uses is taken out of the table: that row
  stops at its first token with it, every other row decodes."""
  levels, streams, tables = _rows_64(golden)
  ac, rows = golden['ac_64'], golden['ac_rows_64']
  users = {}
  for i in range(len(streams)):
    for b in set(ac[rows[i]:rows[i + 1]].tolist()):
      users.setdefault(b, []).append(i)
  lonely = sorted(b for b, who in users.items()
                  if len(who) == 1 and b & 15 and 0 < who[0] < len(streams) - 1)
  assert lonely
  byte = lonely[0]
  bad = users[byte][0]
  table_ac = dict(tables[0])
  del table_ac['%x%x' % (byte >> 4, byte & 15)]
  want = levels.copy()
  want[bad] = 0
  k = 1
  for b in ac[rows[bad]:rows[bad + 1]].tolist():
    if b == byte:
      break
    if b == 0xF0:
      k += 16
      continue
    k += b >> 4
    want[bad, k] = levels[bad, k]
    k += 1
  packed, offsets = pack_strings(streams, 1)
  expect_malformed(device, packed, len(packed), offsets, 64,
                   (table_ac, tables[1]), want, 1, bad)


def test_a_decreasing_offset_pair_is_malformed(golden, device):
  levels, streams, tables = _rows_64(golden)
  packed, offsets = pack_strings(streams, 3)
  offsets[-1] = offsets[-2] - 1
  want = levels.copy()
  want[-1] = 0
  expect_malformed(device, packed, len(packed), offsets, 64, tables, want, 1,
                   len(streams) - 1)


def test_a_table_that_is_not_prefix_free_decodes_nothing(golden, device):
  """status[2] names the smallest symbol id involved; levels is all zero."""
  from utils import jpeg
  levels, streams, tables = _rows_64(golden)
  packed, offsets = pack_strings(streams)
  for clash, want_id in (
      ({'02': tables[0]['01'] + '0'}, 0x01),          # 01 is a prefix of 02
      ({'05': tables[0]['03']}, 0x03)):               # 03 and 05 are equal
    table_ac = dict(tables[0])
    table_ac.update(clash)
    got, status = fenced_unpack(device, packed, len(packed), offsets, 64,
                                (table_ac, tables[1]))
    assert status == [0, 0, want_id + 1]
    assert not got.any()
    with pytest.raises(ValueError):
      jpeg.unpack_streams(helpers.to_dev(packed, device),
                          helpers.to_dev(offsets, device), 64, table_ac,
                          tables[1])
  table_dc = dict(tables[1])
  table_dc['3'] = table_dc['2']
  got, status = fenced_unpack(device, packed, len(packed), offsets, 64,
                              (tables[0], table_dc))
  assert status == [0, 0, 256 + 2 + 1] and not got.any()


def test_error_mapping_on_the_device(golden, device):
  from utils import jpeg
  _, streams, tables = _rows_64(golden)
  packed, offsets = pack_strings(streams)
  p, o = helpers.to_dev(packed, device), helpers.to_dev(offsets, device)
  # a leaf of the code tree grown to 65 bits: still prefix-free
  long_ac = dict(tables[0])
  symbol = [k for k, w in long_ac.items() if set(w) == {'1'}][0]
  long_ac[symbol] = long_ac[symbol].ljust(65, '0')
  jpeg.check_prefix_free(long_ac)
  with pytest.raises(NotImplementedError):
    jpeg.unpack_streams(p, o, 64, long_ac, tables[1])
  with pytest.raises(ValueError):
    jpeg.unpack_streams(p, o, 0, *tables)
  with pytest.raises(ValueError):
    jpeg.unpack_streams(p, o, 4097, *tables)
  with pytest.raises(TypeError):
    jpeg.unpack_streams(p.to(torch.int32), o, 64, *tables)


# ------------------------------------------------- the reference's interface
def test_parse_inverts_generate_jpg_binary_stream(golden, device):
  from utils import jpeg
  for tag, rows in (('64', [25, 31, 40]), ('130', [25, 50]), ('1', [3, 40]),
                    ('300', [28, 45])):
    levels = golden['levels_' + tag].astype(np.int64)
    streams = _strings(golden['streams_' + tag])
    tables = _tables(golden, tag)
    s = levels.shape[1]
    zero = (np.arange(s) % 5 + 40000).astype(np.int64)
    for row in rows:
      inds = torch.from_numpy(levels[row] + zero).to(device)
      stream = jpeg.generate_jpg_binary_stream(inds, zero, False, *tables)
      assert stream == streams[row]
      for zero_arg in (zero, torch.from_numpy(zero).to(device)):
        back = jpeg.parse_jpg_binary_stream(stream, s, zero_arg, *tables)
        assert back.dtype == torch.int64 and tuple(back.shape) == (s,)
        assert torch.equal(back, inds)
  with pytest.raises(ValueError):
    jpeg.parse_jpg_binary_stream(streams[45][:-1], 300, zero, *tables)


def test_decode_patches_gives_the_reconstruction_of_the_rd_point(golden,
                                                                 device):
  """From the bytes alone: bit-equal to apply_filter(dequantize(levels)) and
  the pSNR rate_distortion_point returns -- the levels are identical."""
  from analysis_transforms.fully_connected import invertible_linear
  from utils import jpeg, plotting
  patches = helpers.to_dev(golden['rd_patches'], device)
  dictionary = helpers.to_dev(golden['rd_dictionary'], device)
  widths, order = golden['binwidths'], golden['rd_order']
  for n, multiplier in enumerate(golden['rd_multipliers'].tolist()):
    bpp, psnr, tables = jpeg.rate_distortion_point(
        patches, dictionary, widths, multiplier, order=order)
    levels = helpers.to_dev(golden['rd_levels_%d' % n].astype(np.int32),
                            device)
    packed, offsets = jpeg.pack_streams(levels, *tables)
    assert int(offsets[-1]) == int(golden['rd_total_bits_%d' % n])
    back = _twice(lambda: jpeg.decode_patches(
        packed, offsets, dictionary, widths, multiplier, tables, order=order))
    want = invertible_linear.apply_filter(
        jpeg.dequantize(levels, widths * multiplier, order), dictionary)
    assert back.dtype == torch.float32 and torch.equal(back, want)
    assert plotting.compute_pSNR(patches, back) == psnr
