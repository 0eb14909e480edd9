"""
Writes tests/golden/jpeg.npz by running the REFERENCE's utils/jpeg.py and
utils/matrix_zigzag.py on the levels built below.

  python tools/make_jpeg_golden.py /path/to/vision_transform_codes

The argument is the reference's package directory (the one that holds
utils/); its two modules are imported from there, nothing of them is restated
here.  CPU only, deterministic (numpy.random.RandomState).

What the file holds (allow_pickle=False throughout; strings are stored as
fixed-width byte strings):

  lengths                     the patch lengths s of the per-length cases
  levels_<s>                  int32 (rows, s): random rows at densities 0,
                              0.02, 0.1, 0.5, 1 (v[0] = 0 in a third of them)
                              followed by the constructed rows of
                              constructed_rows()
  ac_<s>, ac_rows_<s>         the reference's AC symbol lists of all rows,
                              flattened as bytes run << 4 | size, and the
                              row offsets into them
  dc_<s>                      the DC category of each row (0 for '-')
  streams_<s>                 the reference's stream of each row under the
                              tables below
  table_{ac,dc}_{symbols,codes}_<s>
                              generate_ac_dc_huffman_tables of levels_<s>, in
                              the order of the reference's dicts
  *_b257                      the same for 257 rows of 64 (density 0.1)
  levels_b5000 (int16), counts_ac_b5000, counts_dc_b5000, bits_b5000,
  table_*_b5000               5000 rows of 64: symbol histograms and len() of
                              each stream, no streams
  ties_counts_*, ties_table_* a count table with many weight-1 ties and its
                              code
  zigzag_in_<v>x<h>, zigzag_out_<v>x<h>, zigzag_back_<v>x<h>
                              zigzag of a matrix of distinct values and
                              inverse_zigzag of that scan
  binwidths                   get_jpeg_quant_hifi_binwidths()
  rd_*                        512 patches of 8 x 8, an orthonormal DCT
                              dictionary, and for each multiplier the float64
                              levels np.rint(codes[:, order] / widths) and
                              the total of the reference's stream lengths
                              under tables trained on those levels.  Patches
                              whose float64 codes come within RD_TIE_MARGIN
                              bins of a rounding tie are redrawn, so that a
                              float32 code does not round to another level.
"""
import pathlib
import sys

import numpy as np

REPO = pathlib.Path(__file__).resolve().parent.parent
LENGTHS = [1, 2, 17, 18, 63, 64, 65, 130, 300]
DENSITIES = [0.0, 0.02, 0.1, 0.5, 1.0]
ROWS_PER_DENSITY = 6
RUNS = [15, 16, 17, 31, 32, 33, 255]
RD_MULTIPLIERS = [1.0, 4.0]
RD_TIE_MARGIN = 0.004


def random_rows(rs, rows, s, density, scale=6.0):
  mags = np.rint(rs.laplace(scale=scale, size=(rows, s))).astype(np.int32)
  mags[mags == 0] = 1
  out = mags * (rs.rand(rows, s) < density)
  out[::3, 0] = 0                       # no DC in a third of the rows
  return out.astype(np.int32)


def magnitudes():
  """+-(2^k - 1) and +-2^k for k = 0..14."""
  values = []
  for k in range(15):
    for m in ((1 << k) - 1, 1 << k):
      values += [m, -m]
  return values


def constructed_rows(s):
  rows = []

  def row(pairs):
    r = np.zeros(s, dtype=np.int32)
    for i, v in pairs:
      if not 0 <= i < s:
        return
      r[i] = v
    rows.append(r)

  row([])                                       # all zero
  row([(0, -7)])                                # only v[0]
  row([(s - 1, 3)])                             # last nonzero at s - 1
  row([(0, 2), (s - 1, -1)])
  for z in RUNS:
    row([(1, 5), (z + 2, -9)])                  # z zeros between two levels
    row([(z + 1, 4)])                           # z zeros from index 1, no DC
    row([(0, -3), (z + 1, 4)])                  # the same behind a DC level
    row([(0, 1), (3, 1), (z + 4, 2), (2 * z + 5, -2)])
  row([(60, 1), (70, -1)])                      # run across lanes 63 | 64
  row([(63, 1), (64, 2)])
  row([(3, -6), (129, 6)])                      # run across a whole chunk
  row([(10, 1), (266, 1), (299, -300)])
  values = magnitudes()
  for start in range(0, len(values), s):        # every magnitude, DC included
    chunk = values[start:start + s]
    row(list(enumerate(chunk)))
  for start in range(0, len(values), max(1, s - 1)):   # and behind a zero DC
    chunk = values[start:start + s - 1]
    if s > 1:
      row([(i + 1, v) for i, v in enumerate(chunk)])
  return np.stack(rows)


def dct_dictionary():
  """(64, 64) float64: row u * 8 + v is the orthonormal 2-d DCT-II basis
  function (u, v) of an 8 x 8 patch, flattened row-major."""
  k = np.arange(8)
  c = np.sqrt(2.0 / 8) * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)
  c[0] = np.sqrt(1.0 / 8)
  return np.einsum('uy,vx->uvyx', c, c).reshape(64, 64)


def as_bytes(strings):
  return np.array([s.encode('ascii') for s in strings] or [b''], dtype='S')


def main(reference_dir):
  sys.dont_write_bytecode = True
  sys.path.insert(0, str(reference_dir))
  from utils import jpeg as ref_jpeg
  from utils import matrix_zigzag as ref_zigzag
  assert pathlib.Path(ref_jpeg.__file__).resolve().parent.parent == (
      pathlib.Path(reference_dir).resolve()), ref_jpeg.__file__

  out = {'lengths': np.array(LENGTHS, dtype=np.int32)}

  def dc_category(symbol):
    return 0 if symbol == '-' else int(symbol, 16)

  def symbols_of(levels):
    zero = np.zeros(levels.shape[1], dtype=np.int64)
    ac, ac_rows, dc = [], [0], []
    for r in levels.astype(np.int64):
      ac_symbols, dc_symbol = ref_jpeg.generate_jpg_binary_stream(r, zero, True)
      ac += [int(x, 16) for x in ac_symbols]
      ac_rows.append(len(ac))
      dc.append(dc_category(dc_symbol))
    return (np.array(ac, dtype=np.uint8), np.array(ac_rows, dtype=np.int64),
            np.array(dc, dtype=np.uint8))

  def tables_of(levels, tag):
    zero = np.zeros(levels.shape[1], dtype=np.int64)
    table_ac, table_dc = ref_jpeg.generate_ac_dc_huffman_tables(
        levels.astype(np.int64), zero)
    for name, table in (('ac', table_ac), ('dc', table_dc)):
      out['table_%s_symbols_%s' % (name, tag)] = as_bytes(list(table.keys()))
      out['table_%s_codes_%s' % (name, tag)] = as_bytes(list(table.values()))
    return table_ac, table_dc

  def streams_of(levels, tables):
    zero = np.zeros(levels.shape[1], dtype=np.int64)
    return [ref_jpeg.generate_jpg_binary_stream(r, zero, False, tables[0],
                                                tables[1])
            for r in levels.astype(np.int64)]

  def whole_case(levels, tag):
    out['levels_' + tag] = levels
    out['ac_' + tag], out['ac_rows_' + tag], out['dc_' + tag] = symbols_of(
        levels)
    out['streams_' + tag] = as_bytes(streams_of(levels, tables_of(levels,
                                                                  tag)))

  for s in LENGTHS:
    rs = np.random.RandomState(1000 + s)
    blocks = [random_rows(rs, ROWS_PER_DENSITY, s, density)
              for density in DENSITIES]
    whole_case(np.concatenate(blocks + [constructed_rows(s)]), str(s))

  whole_case(random_rows(np.random.RandomState(257), 257, 64, 0.1), 'b257')

  big = random_rows(np.random.RandomState(5000), 5000, 64, 0.15, scale=3.0)
  big[7::50] = random_rows(np.random.RandomState(5001), 100, 64, 1.0, 400.0)
  assert np.abs(big).max() <= 32767
  out['levels_b5000'] = big.astype(np.int16)
  ac, _, dc = symbols_of(big)
  out['counts_ac_b5000'] = np.bincount(ac, minlength=256).astype(np.int64)
  out['counts_dc_b5000'] = np.bincount(dc, minlength=16).astype(np.int64)
  out['bits_b5000'] = np.array(
      [len(x) for x in streams_of(big, tables_of(big, 'b5000'))],
      dtype=np.int32)

  # many weight-1 ties next to a few heavy symbols
  ties = {'%x%x' % (r, z): 1 for r in range(15) for z in range(10)}
  ties.update({'00': 900, '01': 400, '11': 400, '02': 7, 'f0': 2, '-': 1})
  table = ref_jpeg.compute_huffman_table(dict(ties))
  out['ties_counts_symbols'] = as_bytes(list(ties.keys()))
  out['ties_counts_weights'] = np.array(list(ties.values()), dtype=np.int64)
  out['ties_table_symbols'] = as_bytes(list(table.keys()))
  out['ties_table_codes'] = as_bytes(list(table.values()))

  for v, h in ((8, 8), (3, 5), (1, 7), (16, 16)):
    matrix = np.random.RandomState(v * 100 + h).permutation(v * h).reshape(
        v, h) + 1.0
    scan = ref_zigzag.zigzag(matrix)
    tag = '%dx%d' % (v, h)
    out['zigzag_in_' + tag] = matrix
    out['zigzag_out_' + tag] = scan
    out['zigzag_back_' + tag] = ref_zigzag.inverse_zigzag(scan, v, h)
  binwidths = ref_jpeg.get_jpeg_quant_hifi_binwidths()
  out['binwidths'] = binwidths

  # ---- rate-distortion case
  rs = np.random.RandomState(512)
  dictionary = dct_dictionary()
  dictionary32 = dictionary.astype(np.float32)
  order = np.array([int(i) for i in ref_zigzag.zigzag(
      np.arange(64).reshape(8, 8))], dtype=np.int32)
  spectrum = 300.0 / (1.0 + np.add.outer(np.arange(8), np.arange(8))) ** 2

  def draw(count):
    coefficients = rs.laplace(size=(count, 64)) * spectrum.reshape(-1)
    coefficients[:, 0] += 1024.0
    return (coefficients @ dictionary).astype(np.float32)

  def near_tie(patches):
    codes = patches.astype(np.float64) @ np.linalg.inv(
        dictionary32.astype(np.float64))
    bad = np.zeros(len(patches), dtype=bool)
    for m in RD_MULTIPLIERS:
      q = codes[:, order] / (binwidths * m)
      bad |= (np.abs(np.abs(q - np.floor(q)) - 0.5) < RD_TIE_MARGIN).any(1)
    return bad

  patches = draw(512)
  for _ in range(200):
    bad = near_tie(patches)
    if not bad.any():
      break
    patches[bad] = draw(int(bad.sum()))
  assert not near_tie(patches).any()
  out['rd_patches'] = patches
  out['rd_dictionary'] = dictionary32
  out['rd_order'] = order
  out['rd_multipliers'] = np.array(RD_MULTIPLIERS)
  codes = patches.astype(np.float64) @ np.linalg.inv(
      dictionary32.astype(np.float64))
  for n, m in enumerate(RD_MULTIPLIERS):
    levels = np.rint(codes[:, order] / (binwidths * m)).astype(np.int32)
    out['rd_levels_%d' % n] = levels.astype(np.int16)
    streams = streams_of(levels, tables_of(levels, 'rd%d' % n))
    out['rd_total_bits_%d' % n] = np.array(sum(len(x) for x in streams),
                                           dtype=np.int64)

  target = REPO / 'tests' / 'golden' / 'jpeg.npz'
  np.savez_compressed(target, **out)
  print('wrote', target, target.stat().st_size, 'bytes')


if __name__ == '__main__':
  main(sys.argv[1])
