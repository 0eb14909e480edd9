"""The device half of the baseline JFIF reader (csrc/jfif_decode.hip,
utils/jfif.py) against the sequential decoders of tests/jfif_data.py (whole
files; tests/test_jfif_host.py holds it to an outside decoder) and
tests/jfif_decode_data.py (constructed segments), levels and planes compared
bit for bit.

Whole files: the project's own on the smallest shapes that take every path,
and five PIL-written ones (tests/golden/jfif_foreign.npz).  The parallel
decode on inputs that never synchronise by themselves (flat images, noise at
quality 100), on segments that span three workgroups, with every kind of
token across a subsequence boundary and with 16-bit codewords, at segment
lengths around one subsequence and one workgroup.  unstuff_bytes around the
2048-byte tile, dc_accumulate around its 256-element tile, malformed input,
the R-D entry point."""
import numpy as np
import pytest
import torch

import jfif_data as truth
import jfif_decode_data as dd

pytestmark = pytest.mark.gpu

SUBSEQ = dd.SUBSEQ_BYTES


def _jfif():
  from utils import jfif
  return jfif


def _dev(array, device):
  return torch.from_numpy(np.ascontiguousarray(array)).to(device)


# ------------------------------------------------ the project's own files
def _round_trip(device, image, subsampling):
  jfif = _jfif()
  x = _dev(image, device)
  if subsampling is None:
    data, info = jfif.encode_gray(x, 75)
  else:
    data, info = jfif.encode_rgb(x, subsampling, 75)
  decoded, got = jfif.decode_bytes(data)
  assert torch.equal(got['levels'], info['levels'])
  assert torch.equal(decoded, jfif.decode_levels(info))
  assert decoded.dtype == torch.float32 and decoded.shape == x.shape
  assert got['layout']['rows'] == info['layout']['rows']
  assert got['layout']['subsampling'] == info['layout']['subsampling']
  assert got['trailing_bits_are_ones'] and got['rounds'] >= 1
  assert all(np.array_equal(a, b) for a, b in zip(
      got['qtables'], [info['qtables'][min(c, 1)]
                       for c in range(len(got['qtables']))]))
  again, twice = jfif.decode_bytes(data)
  assert torch.equal(again, decoded) and twice['rounds'] == got['rounds']
  return data, decoded


@pytest.mark.parametrize('shape', [(1, 1), (8, 8), (17, 23), (33, 19)])
def test_gray_round_trip(device, shape):
  _round_trip(device, truth.gray_image(*shape), None)


@pytest.mark.parametrize('shape', [(16, 16), (33, 19)])
@pytest.mark.parametrize('sub', [(1, 1), (2, 2)])
def test_colour_round_trip(device, shape, sub):
  _round_trip(device, truth.colour_image(*shape), sub)


def test_read_jpeg_after_write_jpeg(device, tmp_path):
  jfif = _jfif()
  for image, name in ((truth.gray_image(17, 23), 'gray.jpg'),
                      (truth.colour_image(33, 19), 'colour.jpg')):
    path = tmp_path / name
    info = jfif.write_jpeg(str(path), _dev(image, device))
    decoded, got = jfif.read_jpeg(str(path))
    assert torch.equal(got['levels'], info['levels'])
    assert torch.equal(decoded, jfif.decode_levels(info))


# ------------------------------------------------------------ foreign files
@pytest.mark.parametrize('name', sorted(dd.FOREIGN))
def test_foreign_files(device, name):
  jfif = _jfif()
  data = dd.load_foreign()[name]
  want = truth.decode(data)
  decoded, info = jfif.decode_bytes(data)
  assert np.array_equal(info['levels'].cpu().numpy(), want['levels'])
  assert len(info['planes']) == len(want['planes'])
  for got, plane in zip(info['planes'], want['planes']):
    assert truth.color_data.same_bits(got.cpu().numpy(), plane)
  assert info['trailing_bits_are_ones']
  if name == 'gray':
    assert decoded.shape == (64, 96)
    assert torch.equal(decoded, info['planes'][0])
  else:
    sh, sv = want['sampling'][0]
    assert decoded.shape == (64, 96, 3)
    assert truth.color_data.same_bits(
        decoded.cpu().numpy(), truth.merge_rgb(want['planes'], (64, 96),
                                               (sv, sh)))


# ------------------------------------------ inputs that never synchronise
def test_degenerate_synchronisation(device):
  """A flat image (every guess falls between a DC token and an end of block,
  and both tables decode a 0 bit) and noise at quality 100 (no end of block
  ever realigns the coefficient index) converge only as fast as the true
  state walks; a loop that stopped on a count would be seen in the levels."""
  jfif = _jfif()
  cases = (
      ('flat gray', lambda: jfif.encode_gray(
          _dev(truth.flat_image(768, 768), device), 75)),
      ('flat 4:2:0', lambda: jfif.encode_rgb(
          _dev(np.full((512, 512, 3), 90.0, np.float32), device), (2, 2), 75)),
      ('noise', lambda: jfif.encode_gray(
          _dev(truth.noise_image(64, 64), device), 100)))
  for name, encode in cases:
    data, info = encode()
    decoded, got = jfif.decode_bytes(data)
    assert torch.equal(got['levels'], info['levels']), name
    assert torch.equal(decoded, jfif.decode_levels(info)), name
    print('jfif_decode_rounds %-10s %d rounds, %d segment bytes'
          % (name, got['rounds'], info['file_bytes'] - info['header_bytes']))
    assert got['rounds'] >= 3, name


# ------------------------------------------------- constructed segments
def _unpack(device, raw, d, tables):
  """unpack_scan of one chain, twice; (levels as numpy, status)."""
  jfif = _jfif()
  seg = raw if torch.is_tensor(raw) else _dev(
      np.frombuffer(raw, dtype=np.uint8).copy(), device)
  levels, status = jfif.unpack_scan(seg, dd.one_table_layout(d), tables)
  again, status2 = jfif.unpack_scan(seg, dd.one_table_layout(d), tables)
  assert torch.equal(levels, again) and status == status2
  return levels, status


def _device_pack(device, levels):
  jfif = _jfif()
  d = levels.shape[0]
  x = _dev(levels, device)
  pred, sel = dd.chain(d), np.zeros(d, dtype=np.uint8)
  tables = jfif.tables_from_counts(*jfif.symbol_counts(x, pred, sel))
  raw, offsets = jfif.pack_scan(x, pred, sel, tables)
  return raw, tables, int(offsets[-1])


def test_dense_rows_across_three_workgroups(device):
  rs = np.random.RandomState(600)
  d = 800     # 88 bytes a row under the tables of uniform levels
  levels = rs.randint(1, 1024, size=(d, 64)) * rs.choice([-1, 1], size=(d, 64))
  levels = levels.astype(np.int32)
  raw, tables, bits = _device_pack(device, levels)
  assert raw.numel() > 2 * dd.GROUP_BYTES
  got, status = _unpack(device, raw, d, tables)
  assert np.array_equal(got.cpu().numpy(), dd.diffs_of(levels))
  assert status[:3] == [0, d, bits] and status[3] >= 3
  # and with DC prediction undone on the device
  back = _jfif().dc_accumulate(got, dd.one_table_layout(d))
  assert np.array_equal(back.cpu().numpy(), levels)


def test_flat_rows_across_the_workgroup_boundary(device):
  """One DC level, then zeros: blocks of two bits behind a first block of
  odd length, so every guess of both workgroups is off by half a block."""
  d = dd.GROUP_BYTES * 8 // 2 + 5000
  levels = np.zeros((d, 64), dtype=np.int32)
  levels[:, 0] = 3
  raw, tables, bits = _device_pack(device, levels)
  assert [int(tables[0]['dc'][0]), int(tables[0]['dc'][2]),
          int(tables[0]['ac'][0])] == [1, 2, 1]
  assert bits == 5 + 2 * (d - 1) and raw.numel() > dd.GROUP_BYTES
  got, status = _unpack(device, raw, d, tables)
  assert status[:3] == [0, d, bits]
  assert status[3] > 256     # never synchronises: one round per subsequence
  got = got.cpu().numpy()
  assert got[0, 0] == 3 and not got[1:].any() and not got[0, 1:].any()


def test_every_token_kind_across_a_subsequence_boundary(device):
  rows = np.concatenate([dd.token_rows()] * 4)
  filler = np.zeros((40, 64), dtype=np.int32)
  _, tables, _ = dd.pack_host(np.concatenate([filler, rows]))
  seen = set()
  for k in range(0, 33):
    levels = np.concatenate([filler[:k], rows])
    d = levels.shape[0]
    raw, _, offsets = dd.pack_host(levels, tables)
    assert len(raw) > 5 * SUBSEQ
    for start, code_end, end, ends_block in dd.token_spans(levels, tables):
      for boundary in range(8 * SUBSEQ, int(offsets[-1]), 8 * SUBSEQ):
        if start < boundary < code_end:
          seen.add('codeword')
        if code_end < boundary < end and end - code_end > 1:
          seen.add('value bits')
        if ends_block and end == boundary:
          seen.add('block end at the boundary')
        if ends_block and start < boundary < end:
          seen.add('block end across the boundary')
    got, status = _unpack(device, raw, d, tables)
    assert np.array_equal(got.cpu().numpy(), dd.diffs_of(levels)), k
    assert status[:3] == [0, d, int(offsets[-1])], k
  assert seen == {'codeword', 'value bits', 'block end at the boundary',
                  'block end across the boundary'}


def test_sixteen_bit_codewords(device):
  tables = dd.geometric_tail_tables()
  rows = []
  for run in (0, 3, 9, 15):
    for size in range(1, 11):
      row = np.zeros(64, dtype=np.int32)
      row[0] = size - 5
      row[1 + run] = (1 << size) - 1
      row[40 + run] = -(1 << (size - 1))
      rows.append(row)
  levels = np.stack(rows)
  used = {run << 4 | size for run in (0, 3, 9, 15) for size in range(1, 11)}
  assert max(int(tables[0]['ac'][s]) for s in used) == 16
  raw, _, offsets = dd.pack_host(levels, tables)
  got, status = _unpack(device, raw, len(rows), tables)
  assert np.array_equal(got.cpu().numpy(), dd.diffs_of(levels))
  assert status[:3] == [0, len(rows), int(offsets[-1])]


@pytest.fixture(scope='module')
def long_segment():
  """A segment of a little over one workgroup, its tables, and the rows."""
  rs = np.random.RandomState(256)
  d = 1500
  levels = (rs.randint(-200, 201, size=(d, 64)) *
            (rs.rand(d, 64) < 0.35)).astype(np.int32)
  levels[:, 0] = rs.randint(-800, 801, size=d)
  raw, tables, _ = dd.pack_host(levels)
  assert len(raw) > dd.GROUP_BYTES + 1
  return raw, tables, dd.diffs_of(levels)


@pytest.mark.parametrize('n', [1, SUBSEQ - 1, SUBSEQ, SUBSEQ + 1,
                               dd.GROUP_BYTES - 1, dd.GROUP_BYTES,
                               dd.GROUP_BYTES + 1])
def test_segment_lengths(device, long_segment, n):
  """A prefix of n bytes: the stream ends inside a block, and what was
  complete before is the sequential decoder's."""
  raw, tables, diffs = long_segment
  d = diffs.shape[0]
  arrays = dd.table_arrays(tables)
  want, want_status = dd.sequential_unpack(raw[:n], [0], [0], arrays, d)
  got, status = _unpack(device, raw[:n], d, tables)
  assert status[:3] == want_status
  done = status[1]
  assert status[2] == -1 and 0 <= done < d
  if status[0]:    # the last token ran into the ones behind the end
    assert status[0] - 1 >= 8 * n - 16
  assert n < 200 or done > 0
  got = got.cpu().numpy()
  assert np.array_equal(got[:done], want[:done])
  assert np.array_equal(got[:done], diffs[:done])
  # exactly the rows that fit: the stream ends where the sequence says
  rows_only, status = _unpack(device, raw[:n], max(done, 1), tables)
  if done:
    assert status[:2] == [0, done] and 0 < status[2] <= 8 * n
    assert np.array_equal(rows_only.cpu().numpy(), diffs[:done])


# ------------------------------------------------------------ unstuff_bytes
def _unstuff_both(device, data, capacity=None):
  jfif = _jfif()
  data = bytes(data)
  want, marker_at = dd.unstuff(data)
  x = _dev(np.frombuffer(data, dtype=np.uint8).copy(), device)
  out, length, marker, dropped = jfif.unstuff_bytes(x, capacity)
  again = jfif.unstuff_bytes(x, capacity)
  assert torch.equal(out, again[0]) and again[1:] == (length, marker, dropped)
  room = len(data) if capacity is None else capacity
  assert (length, marker) == (len(want), marker_at)
  assert dropped == max(0, len(want) - room)
  assert out.cpu().numpy().tobytes() == want[:room]
  return want


def _stuffed(n, seed):
  """n bytes without a marker: 0xFF only in FF 00 pairs, many of them."""
  rs = np.random.RandomState(seed)
  raw = rs.randint(0, 255, size=n).astype(np.uint8)
  raw[rs.rand(n) < 0.2] = 0xFF
  return truth.stuff(raw.tobytes())[:n].rstrip(b'\xff')


@pytest.mark.parametrize('n', [0, 1, 2047, 2048, 2049, 4097])
def test_unstuff_bytes_lengths(device, n):
  data = _stuffed(n + 8, n)[:n]
  data = data[:-1] + b'\x01' if data.endswith(b'\xff') else data
  assert len(data) == n
  want = _unstuff_both(device, data)
  assert want == data.replace(b'\xff\x00', b'\xff')
  if n:
    assert _unstuff_both(device, b'\x00' * n) == b'\x00' * n


def _patched(base, at, piece):
  """base with `piece` at `at`, the bytes around it neutral, so that no pair
  is cut and no marker made but what the piece holds."""
  out = bytearray(base)
  lo, hi = max(0, at - 2), min(len(out), at + len(piece) + 2)
  out[lo:hi] = b'\x01' * (hi - lo)
  if lo and out[lo - 1] == 0xFF:
    out[lo - 1] = 0x01
  out[at:at + len(piece)] = piece
  return out


def test_unstuff_bytes_pairs_and_markers(device):
  base = _patched(_stuffed(6000, 11)[:5000], 4998, b'\x01\x01')
  assert dd.unstuff(base)[1] == 5000 and base.count(b'\xff\x00') > 500
  # FF as the last byte of a tile with 00 first in the next
  for tile_end in (2047, 4095):
    pair = _patched(base, tile_end - 1, b'\x05\xff\x00\x06')
    assert pair[tile_end] == 0xFF and pair[tile_end + 1] == 0x00
    want = _unstuff_both(device, pair)
    assert len(want) < len(pair) and dd.unstuff(pair)[1] == len(pair)
  # FF FF 00: the first FF is a marker
  for at in (0, 1, 2046, 2047, 2048, 3000):
    marked = _patched(base, at, b'\xff\xff\x00\x07')
    assert dd.unstuff(marked)[1] == at
    _unstuff_both(device, marked)
  # a lone FF as the last byte
  lone = _patched(base[:4096], 4095, b'\xff')
  assert dd.unstuff(lone)[1] == 4095
  _unstuff_both(device, lone)
  _unstuff_both(device, b'\xff')
  _unstuff_both(device, b'\xff\x00')
  _unstuff_both(device, b'\x00\xff')
  # a RST marker in the middle: marker_at lies there, what follows is not read
  middle = _patched(base, 2501, b'\xff\xd3')
  assert dd.unstuff(middle)[1] == 2501
  _unstuff_both(device, middle)
  # capacity one short, and none at all
  want = _unstuff_both(device, base, len(dd.unstuff(base)[0]) - 1)
  _unstuff_both(device, base, 0)
  assert len(want) < 5000


def test_unstuff_undoes_stuff(device):
  jfif = _jfif()
  rs = np.random.RandomState(5)
  raw = rs.randint(0, 256, size=4097).astype(np.uint8)
  raw[rs.rand(4097) < 0.2] = 0xFF
  raw[[0, 2047, 2048, 4096]] = 0xFF
  x = _dev(raw, device)
  stuffed, length, dropped = jfif.stuff_bytes(x)
  assert dropped == 0 and length > 4097
  out, back, marker_at, dropped = jfif.unstuff_bytes(stuffed)
  assert (back, marker_at, dropped) == (4097, length, 0)
  assert torch.equal(out, x)


# ------------------------------------------------------------ dc_accumulate
def _accumulate_both(device, levels, order, start):
  jfif = _jfif()
  layout = {'order': order, 'start': start}
  want = dd.dc_accumulate(levels, order, start)
  got = jfif.dc_accumulate(_dev(levels, device), layout)
  assert np.array_equal(got.cpu().numpy(), want)
  return want


@pytest.mark.parametrize('d', [1, 63, 64, 65, 255, 256, 257, 513, 70000])
def test_dc_accumulate_sizes(device, d):
  rs = np.random.RandomState(d)
  levels = rs.randint(-2047, 2048, size=(d, 64)).astype(np.int32)
  order = rs.permutation(d).astype(np.int32)
  start = (rs.rand(d) < 0.02).astype(np.uint8)
  start[0] = 1
  want = _accumulate_both(device, levels, order, start)
  assert np.array_equal(want[:, 1:], levels[:, 1:])
  # one chain: a plain running sum
  start[1:] = 0
  want = _accumulate_both(device, levels, np.arange(d, dtype=np.int32), start)
  assert np.array_equal(want[:, 0], np.cumsum(levels[:, 0]))


def test_dc_accumulate_chains_of_a_420_scan(device):
  jfif = _jfif()
  lay = jfif.frame_layout((33, 19), [(2, 2), (1, 1), (1, 1)])
  rs = np.random.RandomState(3319)
  levels = rs.randint(-900, 901, size=(lay['rows'], 64)).astype(np.int32)
  diffs = levels.copy()
  linked = lay['pred'] >= 0
  diffs[linked, 0] -= levels[lay['pred'][linked], 0]
  want = _accumulate_both(device, diffs, lay['order'], lay['start'])
  assert np.array_equal(want, levels)


def test_dc_accumulate_wraps_and_skips(device):
  d = 300
  levels = np.zeros((d, 64), dtype=np.int32)
  levels[:, 0] = 2 ** 31 - 1
  levels[:, 5] = 7
  order = np.arange(d, dtype=np.int32)
  start = np.zeros(d, dtype=np.uint8)
  want = _accumulate_both(device, levels, order, start)   # no start at all
  assert want[1, 0] == -2 and want[2, 0] == 2 ** 31 - 3
  # entries outside [0, d) add nothing and write nothing
  order[[3, 100, 256, 299]] = (-1, d, 2 ** 31 - 1, -2 ** 31)
  want = _accumulate_both(device, levels, order, start)
  assert (want[[3, 100, 256, 299], 0] == 2 ** 31 - 1).all()


# ----------------------------------------------------------- malformed input
def test_half_a_segment(device):
  jfif = _jfif()
  image = truth.gray_image(64, 48)
  data, info = jfif.encode_gray(_dev(image, device), 75)
  hdr = jfif.parse_headers(data)
  at = hdr['segment_at']
  half = at + (len(data) - 2 - at) // 2
  with pytest.raises(ValueError):
    jfif.decode_bytes(data[:half] + b'\xff\xd9')
  seg, _ = dd.unstuff(data[at:half])
  levels, status = jfif.unpack_scan(
      _dev(np.frombuffer(seg, dtype=np.uint8).copy(), device), info['layout'],
      hdr['tables'], hdr['selectors'])
  done = status[1]
  assert 0 < done < info['layout']['rows'] and status[2] == -1
  if status[0]:     # the ones behind the end read as a malformed token
    assert status[0] - 1 >= 8 * len(seg) - 16
  jfif.dc_accumulate(levels, jfif.frame_layout(hdr['shape'], hdr['sampling']))
  assert torch.equal(levels[:done], info['levels'][:done])


def test_a_table_that_lacks_a_used_symbol(device):
  rs = np.random.RandomState(77)
  d = 400
  levels = (rs.randint(-15, 16, size=(d, 64)) *
            (rs.rand(d, 64) < 0.3)).astype(np.int32)
  levels[:, 0] = rs.randint(-30, 31, size=d)
  # the only AC level of size 6 and the only DC differences of size 10
  levels[250, 30:34] = (1, 0, 0, 40)
  levels[300, 0] = 900
  raw, tables, offsets = dd.pack_host(levels)
  assert len(raw) > 20 * SUBSEQ
  assert tables[0]['ac'][0x26] and tables[0]['dc'][10]
  for kind, symbol, row in (('ac', 0x26, 250), ('dc', 10, 300)):
    # the codewords stay what they were: only the symbol's length goes
    arrays = dd.table_arrays(tables)
    arrays[kind + '_len'][0, symbol] = 0
    want, want_status = dd.sequential_unpack(raw, [0], [0], arrays, d)
    assert want_status[0] > 0 and want_status[1] == row
    jfif = _jfif()
    dev = jfif._DecodeTables(tables, device)
    getattr(dev, kind + '_len')[0, symbol] = 0
    levels_dev, status = _unpack(device, raw, d, dev)
    assert status[:3] == want_status
    done = status[1]
    assert offsets[done] < status[0] <= offsets[done + 1]
    got = levels_dev.cpu().numpy()
    assert np.array_equal(got[:done], want[:done])
    assert np.array_equal(got[:done], dd.diffs_of(levels)[:done])


def test_bytes_that_are_no_stream_at_all(device):
  """Random bytes under tables that cover little: whatever happens is
  reported in status, and the call returns."""
  rs = np.random.RandomState(9)
  tables = [{'dc': np.array([2, 2, 2] + [0] * 13), 'ac': np.array(
      [2, 3, 3] + [0] * 253)}, None]
  arrays = dd.table_arrays(tables)
  for n in (1, 300, dd.GROUP_BYTES + 77):
    raw = rs.randint(0, 256, size=n).astype(np.uint8).tobytes()
    want, want_status = dd.sequential_unpack(raw, [0], [0], arrays, 50)
    got, status = _unpack(device, raw, 50, tables)
    assert status[:3] == want_status
    done = status[1]
    assert np.array_equal(got.cpu().numpy()[:done], want[:done])


def test_tables_that_are_not_prefix_free(device):
  """vtc_jfif_unpack reports no bad table: it decodes by the rule of its decode
  tables (dd.decode_table_rule), the same bits at every call.  One workgroup,
  three subsequences.  The expectation was fixed on the commit before the
  decode table was stated once (csrc/prefix_table.h), which gave status
  [0, 16, 864, 1] and these levels: profiles/prefix_table_refactor.txt."""
  jfif = _jfif()
  rows = 16
  arrays = dd.overlapping_tables()
  raw = dd.overlapping_segment(arrays, rows, seed=26)
  assert 2 * SUBSEQ < len(raw) <= 3 * SUBSEQ
  rule, seen = dd.decode_table_rule(arrays), set()

  def recording(kind, t, w):
    hit = rule(kind, t, w)
    seen.add((kind, hit[0]))
    return hit
  want, want_status = dd.sequential_unpack(raw, [0], [0], arrays, rows,
                                           recording)
  # the walk completes, and meets: the prefix where only longer codewords
  # share its lookup entries, the longer one where both claim them, the twin
  # (the later of two equal keys), a plain predecessor search
  assert want_status[0] == 0 and want_status[1] == rows
  assert {('ac', dd.OVERLAP_PREFIX), ('ac', dd.OVERLAP_LONGER),
          ('ac', dd.OVERLAP_TWIN), ('ac', 0x41)} <= seen
  assert ('ac', dd.OVERLAP_FIRST) not in seen and ('ac', 0x05) not in seen
  # a decoder that takes the shortest match reads other levels
  assert not np.array_equal(
      want, dd.sequential_unpack(raw, [0], [0], arrays, rows)[0])
  dev = jfif._DecodeTables([None, None], device)
  for name in ('ac_code', 'dc_code'):
    setattr(dev, name, _dev(arrays[name].view(np.int16), device))
  for name in ('ac_len', 'dc_len'):
    setattr(dev, name, _dev(arrays[name], device))
  got, status = _unpack(device, raw, rows, dev)   # two calls, equal bits
  print('status', status, 'want', want_status)
  assert status[:3] == want_status
  assert np.array_equal(got.cpu().numpy(), want)


# -------------------------------------------------------------- R-D point
def test_rate_distortion_image_from_stream(device):
  jfif = _jfif()
  for image, sub in ((truth.gray_image(64, 48), None),
                     (truth.colour_image(33, 19), (2, 2))):
    x = _dev(image, device)
    kwargs = {} if sub is None else {'subsampling': sub}
    plain = jfif.rate_distortion_image(x, 75, **kwargs)
    streamed = jfif.rate_distortion_image(x, 75, from_stream=True, **kwargs)
    for key in ('bits_per_pixel', 'pSNR', 'SSIM'):
      assert plain[key] == streamed[key], key
    assert plain['bytes'] == streamed['bytes']
    assert streamed['info']['decoded_from'] == 'bytes'
    assert 'decoded_from' not in plain['info']
