"""The baseline JFIF writer of utils/jfif.py and include/ext/vtc_jfif.h,
restated in numpy (float64, no torch) operation for operation, and an
independent baseline decoder for the files it writes.

Encoder: padding by replication, rint(clip) - 128, the separable DCT with its
sums in ascending k (rows, then columns), np.rint(coefficient / q), the T.81
symbols with DC prediction, package-merge lengths with the all-ones codeword
reserved, canonical codes, the bit string with its pad bits, byte stuffing,
the header segments.  The device's bytes are compared with these by ==.

Decoder: marker parsing, DHT to a decode table, unstuffing, DC prediction,
dequantisation, float64 IDCT (columns, then rows), rint, clamp.  It shares no
code with the encoder but the DCT basis and the zig-zag positions.

The colour step is that of tests/color_data.py (already held to the device
bit for bit by tests/test_color_gpu.py).
"""
import numpy as np

import color_data

ZIGZAG = color_data.zigzag_positions(8)   # [(v, u)] in scan order
ANNEX_K1 = np.array([[16, 11, 10, 16, 24, 40, 51, 61],
                     [12, 12, 14, 19, 26, 58, 60, 55],
                     [14, 13, 16, 24, 40, 57, 69, 56],
                     [14, 17, 22, 29, 51, 87, 80, 62],
                     [18, 22, 37, 56, 68, 109, 103, 77],
                     [24, 35, 55, 64, 81, 104, 113, 92],
                     [49, 64, 78, 87, 103, 121, 120, 101],
                     [72, 92, 95, 98, 112, 100, 103, 99]])
ANNEX_K2 = color_data.ANNEX_K2


def basis():
  u = np.arange(8, dtype=np.float64)[:, None]
  k = np.arange(8, dtype=np.float64)[None, :]
  scale = np.where(u == 0, 1.0 / np.sqrt(2.0), 1.0)
  return scale / 2.0 * np.cos((2.0 * k + 1.0) * u * np.pi / 16.0)


def to_zigzag(natural):
  """(..., 8, 8) -> (..., 64) in scan order."""
  return np.stack([natural[..., v, u] for v, u in ZIGZAG], axis=-1)


def from_zigzag(scan):
  out = np.zeros(scan.shape[:-1] + (8, 8), dtype=scan.dtype)
  for i, (v, u) in enumerate(ZIGZAG):
    out[..., v, u] = scan[..., i]
  return out


# ------------------------------------------------------------------- tables
def quality_tables(quality):
  out = []
  for base in (ANNEX_K1, ANNEX_K2):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    table = (to_zigzag(base).astype(np.int64) * scale + 50) // 100
    out.append(np.clip(table, 1, 255).astype(np.uint16))
  return out


def package_merge(counts, max_len=16, reserve=True):
  """Lengths of the optimal code under max_len; leaves ordered by (weight,
  symbol) with the weight-0 pseudo-symbol first, a leaf before a package of
  equal weight."""
  counts = [int(c) for c in counts]
  leaves = sorted((c, s) for s, c in enumerate(counts) if c > 0)
  lengths = np.zeros(len(counts), dtype=np.int64)
  if not leaves:
    return lengths
  if reserve:
    leaves = [(0, len(counts))] + leaves
  n = len(leaves)
  assert n <= 1 << max_len
  if n == 1:
    lengths[leaves[0][1]] = 1
    return lengths
  singles = [(w, [i]) for i, (w, _) in enumerate(leaves)]
  row = singles
  for _ in range(max_len - 1):
    packages = [(row[j][0] + row[j + 1][0], row[j][1] + row[j + 1][1])
                for j in range(0, len(row) - 1, 2)]
    # stable sort on the weight: singles are listed first, so on a tie a
    # leaf stays in front of a package
    row = sorted(singles + packages, key=lambda item: item[0])
  for _, members in row[:2 * n - 2]:
    for i in members:
      if leaves[i][1] < len(counts):
        lengths[leaves[i][1]] += 1
  return lengths


def canonical(lengths):
  """({symbol: (code, length)}, BITS, HUFFVAL) of T.81 Annex C."""
  order = sorted((int(l), s) for s, l in enumerate(lengths) if l > 0)
  codes, bits, huffval = {}, [0] * 16, []
  code, at = 0, order[0][0] if order else 0
  for length, symbol in order:
    code <<= length - at
    at = length
    codes[symbol] = (code, length)
    code += 1
    bits[length - 1] += 1
    huffval.append(symbol)
  return codes, bits, huffval


# ----------------------------------------------------------------- geometry
def layout(shape, subsampling):
  """Components as dicts, and the scan as a list of (component, by, bx) in
  MCU order."""
  h, w = shape
  if subsampling is None:
    comps = [{'H': 1, 'V': 1, 'tq': 0, 'td': 0}]
  else:
    fv, fh = subsampling
    comps = [{'H': fh, 'V': fv, 'tq': 0, 'td': 0},
             {'H': 1, 'V': 1, 'tq': 1, 'td': 1},
             {'H': 1, 'V': 1, 'tq': 1, 'td': 1}]
  hmax = max(c['H'] for c in comps)
  vmax = max(c['V'] for c in comps)
  mcus_v, mcus_h = -(-h // (8 * vmax)), -(-w // (8 * hmax))
  for c in comps:
    c['shape'] = (-(-h * c['V'] // vmax), -(-w * c['H'] // hmax))
    c['grid'] = (mcus_v * c['V'], mcus_h * c['H'])
  scan = []
  for my in range(mcus_v):
    for mx in range(mcus_h):
      for ci, c in enumerate(comps):
        for dy in range(c['V']):
          for dx in range(c['H']):
            scan.append((ci, my * c['V'] + dy, mx * c['H'] + dx))
  return comps, scan


def scan_arrays(shape, subsampling):
  """(row_of_block per plane, pred, table_sel) as utils.jfif.scan_layout gives
  them, from the scan list."""
  comps, scan = layout(shape, subsampling)
  rob = [np.zeros(c['grid'], dtype=np.int32) for c in comps]
  pred = np.full(len(scan), -1, dtype=np.int32)
  sel = np.zeros(len(scan), dtype=np.uint8)
  last = {}
  for row, (ci, by, bx) in enumerate(scan):
    rob[ci][by, bx] = row
    pred[row] = last.get(ci, -1)
    last[ci] = row
    sel[row] = comps[ci]['td']
  return [r.reshape(-1) for r in rob], pred, sel


# ---------------------------------------------------------------------- DCT
def forward_dct(plane, grid, q):
  """(bh, bw, 64) int32 levels in scan order of a float32 plane."""
  C = basis()
  h, w = plane.shape
  bh, bw = grid
  p = np.asarray(plane, dtype=np.float32).astype(np.float64)
  s = np.rint(np.clip(p, 0.0, 255.0)) - 128.0
  s = s[np.minimum(np.arange(bh * 8), h - 1)][
      :, np.minimum(np.arange(bw * 8), w - 1)]
  s = s.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)    # (bh, bw, y, x)
  t = None
  for k in range(8):    # t[y, u] = sum_k s[y, k] C[u, k]
    prod = s[..., :, k, None] * C[None, None, None, :, k]
    t = prod if k == 0 else t + prod
  c = None
  for k in range(8):    # c[v, u] = sum_k t[k, u] C[v, k]
    prod = t[..., k, None, :] * C[None, None, :, k, None]
    c = prod if k == 0 else c + prod
  qn = from_zigzag(np.asarray(q, dtype=np.float64))
  return to_zigzag(np.rint(c / qn)).astype(np.int32)


def inverse_dct(levels, shape, q):
  """float32 (h, w) plane of (bh, bw, 64) levels."""
  C = basis()
  bh, bw = levels.shape[:2]
  c = from_zigzag(levels.astype(np.float64) * np.asarray(q, dtype=np.float64))
  t = None
  for k in range(8):    # t[y, u] = sum_k c[k, u] C[k, y]
    prod = c[..., k, None, :] * C[None, None, k, :, None]
    t = prod if k == 0 else t + prod
  p = None
  for k in range(8):    # p[y, x] = sum_k t[y, k] C[k, x]
    prod = t[..., :, k, None] * C[None, None, None, k, :]
    p = prod if k == 0 else p + prod
  r = np.clip(np.rint(p + 128.0), 0.0, 255.0)
  full = r.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
  return full[:shape[0], :shape[1]].astype(np.float32)


# ------------------------------------------------------------------ symbols
def bit_length(n):
  return int(abs(int(n))).bit_length()


def value_bits(n, size):
  n = int(n)
  return (n if n >= 0 else n - 1) & ((1 << size) - 1)


def block_tokens(row, previous_dc):
  """[('dc' | 'ac', symbol, value, size)] of one block in stream order;
  ValueError beyond the baseline sizes."""
  diff = int(row[0]) - int(previous_dc)
  size = bit_length(diff)
  if size > 11:
    raise ValueError('DC difference %d' % diff)
  tokens = [('dc', size, value_bits(diff, size), size)]
  run = 0
  for i in range(1, 64):
    v = int(row[i])
    if v == 0:
      run += 1
      continue
    while run >= 16:
      tokens.append(('ac', 0xF0, 0, 0))
      run -= 16
    size = bit_length(v)
    if size > 10:
      raise ValueError('AC level %d' % v)
    tokens.append(('ac', run << 4 | size, value_bits(v, size), size))
    run = 0
  if run:
    tokens.append(('ac', 0x00, 0, 0))
  return tokens


def scan_tokens(levels, pred, sel):
  return [(int(sel[r]), block_tokens(
      levels[r], levels[pred[r]][0] if pred[r] >= 0 else 0))
          for r in range(levels.shape[0])]


def count_symbols(tokens):
  ac = np.zeros((2, 256), dtype=np.int64)
  dc = np.zeros((2, 16), dtype=np.int64)
  for pair, block in tokens:
    for kind, symbol, _, _ in block:
      (dc if kind == 'dc' else ac)[pair, symbol] += 1
  return ac, dc


def build_tables(ac, dc):
  return [None if not (ac[p].any() or dc[p].any()) else
          {'dc': package_merge(dc[p]), 'ac': package_merge(ac[p])}
          for p in range(2)]


def pack_tokens(tokens, tables):
  """(raw bytes with the last byte padded with ones, number of bits, bit
  offset of every block and the total); KeyError for a symbol the tables
  lack."""
  codes = [None if t is None else {'dc': canonical(t['dc'])[0],
                                   'ac': canonical(t['ac'])[0]}
           for t in tables]
  pieces, offsets, at = [], [], 0
  for pair, block in tokens:
    offsets.append(at)
    for kind, symbol, value, size in block:
      code, length = codes[pair][kind][symbol]
      pieces.append(format(code, '0%db' % length))
      if size:
        pieces.append(format(value, '0%db' % size))
      at += length + size
  offsets.append(at)
  bits = ''.join(pieces)
  assert len(bits) == at
  bits += '1' * (-at % 8)
  raw = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
  return raw, at, np.array(offsets, dtype=np.int64)


def stuff(raw):
  return bytes(raw).replace(b'\xff', b'\xff\x00')


# ------------------------------------------------------------------ headers
def _segment(marker, payload):
  return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload


def headers(shape, comps, qtables, tables):
  h, w = shape
  out = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00' + bytes(
      [1, 1, 0, 0, 1, 0, 1, 0, 0]))]
  for i, q in enumerate(qtables):
    out.append(_segment(0xDB, bytes([i]) + bytes(int(v) for v in q)))
  frame = bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big')
  frame += bytes([len(comps)])
  for i, c in enumerate(comps):
    frame += bytes([i + 1, c['H'] << 4 | c['V'], c['tq']])
  out.append(_segment(0xC0, frame))
  for p, t in enumerate(tables):
    if t is None:
      continue
    for klass, key in ((0, 'dc'), (1, 'ac')):
      _, bits, huffval = canonical(t[key])
      out.append(_segment(0xC4, bytes([klass << 4 | p]) + bytes(bits) +
                          bytes(huffval)))
  scan = bytes([len(comps)])
  for i, c in enumerate(comps):
    scan += bytes([i + 1, c['td'] << 4 | c['td']])
  out.append(_segment(0xDA, scan + bytes([0, 63, 0])))
  return b''.join(out)


# ------------------------------------------------------------------ encoder
def encode_planes(planes, shape, subsampling, quality=75, qtables=None):
  """(bytes, info) of float32 planes ([Y] or [Y, Cb, Cr])."""
  comps, scan = layout(shape, subsampling)
  assert [tuple(p.shape) for p in planes] == [c['shape'] for c in comps]
  luma, chroma = quality_tables(quality) if qtables is None else qtables
  qtables = [luma] if len(comps) == 1 else [luma, chroma]
  grids = [forward_dct(p, c['grid'], qtables[c['tq']])
           for p, c in zip(planes, comps)]
  levels = np.stack([grids[ci][by, bx] for ci, by, bx in scan])
  _, pred, sel = scan_arrays(shape, subsampling)
  tokens = scan_tokens(levels, pred, sel)
  ac, dc = count_symbols(tokens)
  tables = build_tables(ac, dc)
  raw, nbits, offsets = pack_tokens(tokens, tables)
  stuffed = stuff(raw)
  head = headers(shape, comps, qtables, tables)
  data = head + stuffed + b'\xff\xd9'
  return data, {'levels': levels, 'grids': grids, 'comps': comps,
                'qtables': qtables, 'tables': tables, 'scan_bits': nbits,
                'raw': raw, 'offsets': offsets, 'ac_counts': ac,
                'dc_counts': dc, 'stuffed_bytes': len(stuffed) - len(raw),
                'header_bytes': len(head) + 2}


def split_rgb(image, subsampling):
  """[Y, Cb, Cr] float32 of an (h, w, 3) float32 RGB image, as
  utils.color.split_planes computes them."""
  ycc = color_data.rgb_to_ycbcr(image[None], out_layout=color_data.CHW)[0]
  chroma = color_data.downsample(ycc[1:], subsampling[0], subsampling[1])
  return [ycc[0], chroma[0], chroma[1]]


def encode_gray(image, quality=75, qtables=None):
  return encode_planes([image], image.shape, None, quality, qtables)


def encode_rgb(image, subsampling=(2, 2), quality=75, qtables=None):
  return encode_planes(split_rgb(image, subsampling), image.shape[:2],
                       subsampling, quality, qtables)


def merge_rgb(planes, shape, subsampling):
  """(h, w, 3) float32 RGB as utils.jfif.decode_levels gives it."""
  chroma = color_data.upsample(np.stack(planes[1:]), subsampling[0],
                               subsampling[1], shape, color_data.TRIANGLE)
  ycc = np.concatenate([planes[0][None], chroma])[None]
  return color_data.ycbcr_to_rgb(ycc, clamp=(0.0, 255.0),
                                 layout=color_data.CHW,
                                 out_layout=color_data.HWC)[0]


# ------------------------------------------------------------------ decoder
class _Bits(object):
  def __init__(self, data):
    self.data, self.at = data, 0

  def bit(self):
    byte = self.data[self.at >> 3]
    self.at += 1
    return byte >> (7 - (self.at - 1 & 7)) & 1

  def take(self, n):
    v = 0
    for _ in range(n):
      v = v << 1 | self.bit()
    return v

  def symbol(self, table):
    code = 0
    for length in range(1, 17):
      code = code << 1 | self.bit()
      if (length, code) in table:
        return table[(length, code)]
    raise ValueError('no codeword matches')


def _extend(value, size):
  """T.81 F.2.2.1 EXTEND."""
  return value if size == 0 or value >> (size - 1) else value - (1 << size) + 1


def decode(data):
  """A baseline decoder.  Returns {'shape', 'levels' (rows in scan order,
  64), 'planes' (float32, one per component at its own resolution),
  'sampling', 'qtables'}."""
  assert data[:2] == b'\xff\xd8'
  at = 2
  qt, ht, frame, scan_comps = {}, {}, None, None
  while True:
    assert data[at] == 0xFF
    marker = data[at + 1]
    size = int.from_bytes(data[at + 2:at + 4], 'big')
    body = data[at + 4:at + 2 + size]
    at += 2 + size
    if marker == 0xDB:
      while body:
        assert body[0] >> 4 == 0    # 8-bit entries
        qt[body[0] & 15] = np.array(list(body[1:65]), dtype=np.int64)
        body = body[65:]
    elif marker == 0xC0:
      assert body[0] == 8
      frame = {'h': int.from_bytes(body[1:3], 'big'),
               'w': int.from_bytes(body[3:5], 'big'), 'comps': []}
      for i in range(body[5]):
        cid, hv, tq = body[6 + 3 * i:9 + 3 * i]
        frame['comps'].append({'id': cid, 'H': hv >> 4, 'V': hv & 15,
                               'tq': tq})
    elif marker == 0xC4:
      while body:
        klass, index = body[0] >> 4, body[0] & 15
        counts = list(body[1:17])
        values = list(body[17:17 + sum(counts)])
        body = body[17 + sum(counts):]
        table, code, k = {}, 0, 0
        for length in range(1, 17):
          for _ in range(counts[length - 1]):
            table[(length, code)] = values[k]
            code += 1
            k += 1
          code <<= 1
        ht[(klass, index)] = table
    elif marker == 0xDA:
      scan_comps = []
      for i in range(body[0]):
        cid, tables = body[1 + 2 * i:3 + 2 * i]
        scan_comps.append((cid, tables >> 4, tables & 15))
      assert list(body[1 + 2 * body[0]:]) == [0, 63, 0]
      break
    else:
      assert 0xE0 <= marker <= 0xEF or marker == 0xFE, hex(marker)
  # every 0xFF of the segment is followed by 0x00: the first FF D9 is EOI
  end = data.index(b'\xff\xd9', at)
  assert end + 2 == len(data)
  segment = data[at:end]
  # no marker inside the segment: every 0xFF is followed by 0x00
  for i, b in enumerate(segment):
    if b == 0xFF:
      assert i + 1 < len(segment) and segment[i + 1] == 0, 'unstuffed 0xFF'
  reader = _Bits(segment.replace(b'\xff\x00', b'\xff'))

  comps = frame['comps']
  assert [c[0] for c in scan_comps] == [c['id'] for c in comps]
  hmax = max(c['H'] for c in comps)
  vmax = max(c['V'] for c in comps)
  mcus_v = -(-frame['h'] // (8 * vmax))
  mcus_h = -(-frame['w'] // (8 * hmax))
  for c in comps:
    c['grid'] = np.zeros((mcus_v * c['V'], mcus_h * c['H'], 64),
                         dtype=np.int32)
    c['dc'] = 0
  rows = []
  for my in range(mcus_v):
    for mx in range(mcus_h):
      for c, (_, td, ta) in zip(comps, scan_comps):
        for dy in range(c['V']):
          for dx in range(c['H']):
            block = np.zeros(64, dtype=np.int32)
            size = reader.symbol(ht[(0, td)])
            c['dc'] += _extend(reader.take(size), size)
            block[0] = c['dc']
            i = 1
            while i < 64:
              rs = reader.symbol(ht[(1, ta)])
              run, size = rs >> 4, rs & 15
              if size == 0:
                if run != 15:
                  break
                i += 16
                continue
              i += run
              block[i] = _extend(reader.take(size), size)
              i += 1
            assert i <= 64
            c['grid'][my * c['V'] + dy, mx * c['H'] + dx] = block
            rows.append(block)
  # what is left of the last byte is padding, all ones
  left = 8 * len(reader.data) - reader.at
  assert 0 <= left < 8 and reader.take(left) == (1 << left) - 1
  planes = []
  for c in comps:
    shape = (-(-frame['h'] * c['V'] // vmax), -(-frame['w'] * c['H'] // hmax))
    planes.append(inverse_dct(c['grid'], shape, qt[c['tq']]))
  return {'shape': (frame['h'], frame['w']), 'levels': np.stack(rows),
          'planes': planes, 'sampling': [(c['H'], c['V']) for c in comps],
          'qtables': [qt[k] for k in sorted(qt)]}


def decode_tables_only(data):
  """{index: int64[64]}: the DQT tables of any JPEG file as they are written,
  in zig-zag order."""
  assert data[:2] == b'\xff\xd8'
  at, out = 2, {}
  while data[at + 1] != 0xDA:
    assert data[at] == 0xFF
    size = int.from_bytes(data[at + 2:at + 4], 'big')
    body = data[at + 4:at + 2 + size]
    if data[at + 1] == 0xDB:
      while body:
        assert body[0] >> 4 == 0
        out[body[0] & 15] = np.array(list(body[1:65]), dtype=np.int64)
        body = body[65:]
    at += 2 + size
  return out


# ------------------------------------------------------------------- inputs
def gray_image(h, w, seed=7):
  """float32 (h, w) in [0, 255]: smooth, with texture and noise, not on the
  integer grid."""
  rs = np.random.RandomState(1000 * seed + 31 * h + w)
  y, x = np.mgrid[0:h, 0:w].astype(np.float64)
  img = (128.0 + 70.0 * np.sin(x / 5.0 + seed) * np.cos(y / 7.0) +
         30.0 * np.sin((x + 2.0 * y) / 2.3) + 12.0 * rs.randn(h, w))
  return np.clip(img, 0.0, 255.0).astype(np.float32)


def flat_image(h, w, value=77.0):
  return np.full((h, w), value, dtype=np.float32)


def noise_image(h, w, seed=5):
  rs = np.random.RandomState(seed)
  return rs.randint(0, 256, size=(h, w)).astype(np.float32)


def colour_image(h, w, seed=3347):
  return color_data.colour_image(h, w, seed)
