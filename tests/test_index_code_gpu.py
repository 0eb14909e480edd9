"""vtc_index_code_bits and vtc_index_code_pack (include/vtc_index_code.h),
utils.index_coding and the source_code='huffman' rate-distortion points
against the restatement of tests/index_code_data.py: integers and bytes, no
tolerances.  Every device call runs twice and its bytes are compared.

The shapes (data.SHAPES) sit at the lane, wave, chunk and block edges of the
kernels' mapping; the tables hold trained codes of 1 to about 18 bits, the
constructed 1 .. 64-bit code with its 32-, 33- and 64-bit words in use, a
one-symbol column and a column with k < kmax; the streams are placed behind
0, 3 and 29 leading bits with gaps between the rows."""
import ctypes

import numpy as np
import pytest
import torch

import fences
import index_code_data as data
import vq_data

pytestmark = pytest.mark.gpu

OK = 0
IDS = ['%dx%d-k%d' % shape for shape in data.SHAPES]


def dev(array, device):
  return torch.from_numpy(np.ascontiguousarray(array)).to(device)


def p(t):
  return ctypes.c_void_p(t.data_ptr())


def twice(fn):
  """fn() twice; the results (tensors, arrays, numbers, tuples of them) must
  agree byte for byte."""
  first, second = fn(), fn()

  def same(a, b):
    if isinstance(a, (tuple, list)):
      return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
      return torch.equal(a, b)
    if isinstance(a, np.ndarray):
      return np.array_equal(a, b)
    return a == b
  assert same(first, second), 'two runs differ'
  return first


def device_tables(device, tables, kmax):
  from utils import index_coding
  code, length = index_coding.index_table_arrays(tables, kmax)
  return dev(code.view(np.int64), device), dev(length, device)


def raw_bits(device, indices, length, kmax):
  """(row_bits, column_bits, status) as numpy arrays, outputs pre-filled with
  a pattern the call has to overwrite."""
  import vtc_hip
  lib = vtc_hip.load_library()
  b, m = indices.shape
  rows = torch.full((b,), -7, dtype=torch.int32, device=device)
  cols = torch.full((m,), -7, dtype=torch.int64, device=device)
  status = torch.full((3,), -7, dtype=torch.int64, device=device)
  rc = lib.vtc_index_code_bits(p(indices), b, m, p(length), kmax, p(rows),
                               p(cols), p(status),
                               vtc_hip.current_stream(device))
  assert rc == OK, lib.vtc_last_error()
  return rows.cpu().numpy(), cols.cpu().numpy(), status.cpu().numpy()


def raw_pack(device, indices, code, length, kmax, offsets, nbytes,
             packed=None):
  """(packed, status) as numpy arrays; `packed` pre-filled with ones."""
  import vtc_hip
  lib = vtc_hip.load_library()
  b, m = indices.shape
  if packed is None:
    packed = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
  packed.fill_(0xFF)
  status = torch.full((3,), -7, dtype=torch.int64, device=device)
  rc = lib.vtc_index_code_pack(p(indices), b, m, p(code), p(length), kmax,
                               p(offsets), p(packed), nbytes, p(status),
                               vtc_hip.current_stream(device))
  assert rc == OK, lib.vtc_last_error()
  return packed.cpu().numpy()[:nbytes], status.cpu().numpy()


# --------------------------------------------------------------- exact bits
@pytest.mark.parametrize('shape', data.SHAPES, ids=IDS)
def test_bits_and_packed_streams(device, shape):
  from utils import index_coding
  from utils import jpeg
  b, m, kmax = shape
  tables, _ = data.case_tables(*shape)
  host = data.case_indices(*shape)
  indices = dev(host, device)
  code, length = device_tables(device, tables, kmax)
  want_rows = data.row_bits(host, tables)
  want_cols = data.column_bits(host, tables)

  rows, cols, status = twice(lambda: raw_bits(device, indices, length, kmax))
  assert np.array_equal(rows, want_rows) and rows.dtype == np.int32
  assert np.array_equal(cols, want_cols) and cols.dtype == np.int64
  assert status.tolist() == [0, 0, 0]

  for lead in data.LEADS:
    offsets = data.layout(want_rows, lead, data.gaps(b))
    nbytes = -(-int(offsets[-1]) // 8)
    want, cut = data.image(host, tables, offsets, nbytes)
    assert cut == 0
    packed, status = twice(lambda: raw_pack(
        device, indices, code, length, kmax, dev(offsets, device), nbytes))
    assert status.tolist() == [0, 0, 0]
    # every stream in its place, every bit outside the rows zero
    assert np.array_equal(packed, want), (shape, lead)

  # the Python interface: offsets from jpeg.bit_offsets, rows read back with
  # jpeg.stream_as_str
  got_rows, got_cols = twice(lambda: index_coding.index_code_bits(indices,
                                                                   tables))
  assert got_rows.dtype == torch.int32 and got_cols.dtype == torch.int64
  assert np.array_equal(got_rows.cpu().numpy(), want_rows)
  assert np.array_equal(got_cols.cpu().numpy(), want_cols)
  packed, offsets = twice(lambda: index_coding.pack_index_streams(indices,
                                                                   tables))
  want_offsets = data.layout(want_rows, 0, [0] * b)
  assert packed.dtype == torch.uint8 and offsets.dtype == torch.int64
  assert np.array_equal(offsets.cpu().numpy(), want_offsets)
  assert packed.numel() == max(1, -(-int(want_offsets[-1]) // 8))
  for r in sorted(set(range(min(b, 70))) | {b - 1}):
    assert jpeg.stream_as_str(packed, offsets, r) == data.stream(host[r],
                                                                 tables), r
  want, _ = data.image(host, tables, want_offsets, packed.numel())
  assert np.array_equal(packed.cpu().numpy(), want)


def test_a_vector_index_column_is_one_dimensional_too(device):
  """indices [b] are (b, 1): what vector_assign returns."""
  from utils import index_coding
  shape = (257, 1, 4096)
  tables, _ = data.case_tables(*shape)
  host = data.case_indices(*shape)
  rows, cols = index_coding.index_code_bits(dev(host[:, 0], device), tables)
  assert np.array_equal(rows.cpu().numpy(), data.row_bits(host, tables))
  assert cols.tolist() == data.column_bits(host, tables).tolist()


# -------------------------------------------------------- uncodable entries
@pytest.mark.parametrize('shape', [(65, 1, 4096), (257, 42, 1024),
                                   (2, 130, 8)],
                         ids=['65x1', '257x42', '2x130'])
def test_uncodable_entries(device, shape):
  """An index of -1, one of kmax and an absent symbol: counted, the first one
  located, no bits; KeyError from Python with the column and the index."""
  from utils import index_coding
  b, m, kmax = shape
  tables, k = data.case_tables(*shape)
  host = data.case_indices(*shape).copy()
  short = data.column_kinds(*shape).index('short') if m > 1 else 0
  absent = k[short] if m > 1 else 65        # past the 65 symbols of 'long'
  assert absent < kmax and absent not in tables[short]
  spots = [(b - 1, m - 1, kmax), (b // 2, short, absent), (b // 3, m // 2, -1)]
  for r, j, value in spots:
    host[r, j] = value
  first = min(r * m + j for r, j, _ in spots)
  assert data.status(host, tables) == [3, 1 + first]
  indices = dev(host, device)
  code, length = device_tables(device, tables, kmax)
  want_rows = data.row_bits(host, tables)

  rows, cols, status = twice(lambda: raw_bits(device, indices, length, kmax))
  assert status.tolist() == [3, 1 + first, 0]
  assert np.array_equal(rows, want_rows)
  assert np.array_equal(cols, data.column_bits(host, tables))
  offsets = data.layout(want_rows, 3, data.gaps(b))
  nbytes = -(-int(offsets[-1]) // 8)
  packed, status = twice(lambda: raw_pack(
      device, indices, code, length, kmax, dev(offsets, device), nbytes))
  assert status.tolist() == [3, 1 + first, 0]
  assert np.array_equal(packed, data.image(host, tables, offsets, nbytes)[0])

  r, j = divmod(first, m)
  for call in (index_coding.index_code_bits, index_coding.pack_index_streams):
    with pytest.raises(KeyError) as error:
      call(indices, tables)
    text = str(error.value)
    assert 'column %d ' % j in text and 'index %d ' % host[r, j] in text, text


# ------------------------------------------------- windows and short buffers
@pytest.mark.parametrize('shape', [(257, 1, 4096), (257, 42, 1024),
                                   (3, 65, 8)],
                         ids=['257x1', '257x42', '3x65'])
def test_a_buffer_one_byte_short(device, shape):
  """The bits past the end are dropped and counted, nothing is written there:
  the packed bytes sit between guard bands."""
  b, m, kmax = shape
  tables, _ = data.case_tables(*shape)
  host = data.case_indices(*shape)
  indices = dev(host, device)
  code, length = device_tables(device, tables, kmax)
  offsets = data.layout(data.row_bits(host, tables), 0, [0] * b)
  total = int(offsets[-1])
  for skew, missing in ((0, 1), (1, 1), (3, 2)):
    nbytes = -(-total // 8) - missing
    assert nbytes > 8
    want, cut = data.image(host, tables, offsets, nbytes)
    assert cut == total - 8 * nbytes > 0
    arena, fence = fences.fenced((nbytes,), torch.uint8, device, skew=skew)
    packed, status = twice(lambda: raw_pack(
        device, indices, code, length, kmax, dev(offsets, device), nbytes,
        packed=arena))
    fence.assert_intact('%s one byte short, skew %d' % (shape, skew))
    assert status.tolist() == [0, 0, cut]
    assert np.array_equal(packed, want)
  # no room at all: every bit dropped, the buffer not touched
  arena, fence = fences.fenced((16,), torch.uint8, device)
  _, status = raw_pack(device, indices, code, length, kmax,
                       dev(offsets, device), 0, packed=arena)
  assert status.tolist() == [0, 0, total]
  assert bool((arena == 0xFF).all())
  fence.assert_intact('%s no room' % (shape,))


def test_windows_cut_rows_and_bad_offsets_drop_them(device):
  """A row may use the bits below offsets[r + 1]: what does not fit is
  dropped and counted; a negative or decreasing offset drops the row; a row
  that starts past the buffer is dropped."""
  shape = (5, 23, 64)
  b, m, kmax = shape
  tables, _ = data.case_tables(*shape)
  host = data.case_indices(*shape)
  bits = data.row_bits(host, tables)
  assert bits.min() > 40
  indices = dev(host, device)
  code, length = device_tables(device, tables, kmax)
  start1 = 7 + int(bits[0]) - 9                # row 0 loses its last 9 bits
  start3 = start1 + int(bits[1]) + 4
  offsets = np.array([7, start1, start3 + 50, start3, start3 + int(bits[3]),
                      start3 + int(bits[3]) + 5], dtype=np.int64)
  # row 2 starts above offsets[3]: dropped; row 4 has 5 bits of room
  nbytes = -(-int(offsets[-1]) // 8)
  want, cut = data.image(host, tables, offsets, nbytes)
  assert cut == 9 + int(bits[2]) + int(bits[4]) - 5
  packed, status = twice(lambda: raw_pack(
      device, indices, code, length, kmax, dev(offsets, device), nbytes))
  assert status.tolist() == [0, 0, cut]
  assert np.array_equal(packed, want)
  negative = np.array([-3, 90, 200, 300, 1 << 40, (1 << 40) + 500], np.int64)
  want, cut = data.image(host, tables, negative, 64)
  assert cut >= int(bits[0]) + int(bits[4])
  packed, status = twice(lambda: raw_pack(
      device, indices, code, length, kmax, dev(negative, device), 64))
  assert status.tolist() == [0, 0, cut]
  assert np.array_equal(packed, want)


# --------------------------------------------------------- rate-distortion
WIDTH, MULT = 5.0, 2.0


@pytest.fixture(scope='module')
def scene(device):
  """The training scene of tests/vq_data.py and a test set with another
  index distribution: the rows in reverse, shrunk, the non-zero codes
  jittered."""
  s = vq_data.scene()
  rs = np.random.RandomState(9)
  codes = s['codes'][::-1].astype(np.float64)
  test_codes = np.where(codes != 0,
                        0.6 * codes + rs.uniform(-30, 30, codes.shape), 0.0)
  on = {'codes': dev(s['codes'], device), 'patches': dev(s['patches'], device),
        'dictionary': dev(s['dictionary'], device),
        'test_codes': dev(test_codes.astype(np.float32), device),
        'test_patches': dev(s['patches'][::-1], device)}
  on['numel'] = s['patches'].size
  return on


def restated_rate(indices, tables, numel):
  host = indices.cpu().numpy()
  assert data.status(host, tables) == [0, 0]
  return int(data.row_bits(host, tables).sum()) / float(numel)


def check_trained(tables, counts, k):
  """Optimal for the weights the rule prescribes, and complete below k."""
  assert len(tables) == len(k) == counts.shape[0]
  for table, row, kj in zip(tables, counts, k):
    weights = data.training_weights(row, int(kj))
    assert sorted(table) == list(range(int(kj)))
    assert data.table_cost(table, weights) == data.huffman_cost(weights)


def test_compute_RD_point_huffman(device, scene):
  from utils import quantization
  codes, patches, dictionary = (scene['codes'], scene['patches'],
                                scene['dictionary'])
  codebook = quantization._uniform_for(codes, [WIDTH] * 64, MULT)
  kmax = codebook[0].shape[1]
  rate, dist, tables = twice(lambda: quantization.compute_RD_point(
      codes, patches, dictionary, codebook, source_code='huffman'))
  entropy_rate, entropy_dist, none = quantization.compute_RD_point(
      codes, patches, dictionary, codebook, source_code='entropy')
  assert none is None and dist == entropy_dist

  indices = quantization.assign(codes, codebook)
  train = indices.cpu().numpy()
  counts = np.stack([np.bincount(train[:, j], minlength=kmax)
                     for j in range(64)])
  check_trained(tables, counts, codebook[1])
  want = restated_rate(indices, tables, scene['numel'])
  print('index_code_rd train huffman %.6f entropy %.6f' % (rate, entropy_rate))
  assert rate == want and rate >= entropy_rate > 0

  # the test set under the trained tables: an out-of-sample rate
  test_indices = quantization.assign(scene['test_codes'], codebook)
  test = test_indices.cpu().numpy()
  unseen = [(r, j) for r in range(test.shape[0]) for j in range(64)
            if counts[j, test[r, j]] == 0]
  assert unseen, 'no test index is new: the weight-1 rule is not exercised'
  want = restated_rate(test_indices, tables, scene['numel'])
  own_entropy = data.entropy_bits(test, kmax) / float(scene['numel'])
  assert want > own_entropy                    # on the CPU first
  test_rate, _, same = twice(lambda: quantization.compute_RD_point(
      scene['test_codes'], scene['test_patches'], dictionary, codebook,
      source_code='huffman', tables=tables))
  assert same is tables and test_rate == want
  device_entropy = quantization.compute_RD_point(
      scene['test_codes'], scene['test_patches'], dictionary, codebook,
      source_code='entropy')[0]
  print('index_code_rd test huffman %.6f own entropy %.6f, %d unseen entries'
        % (test_rate, device_entropy, len(unseen)))
  assert abs(device_entropy - own_entropy) <= 1e-12 * own_entropy
  assert test_rate > device_entropy
  with pytest.raises(ValueError):
    quantization.compute_RD_point(codes, patches, dictionary, codebook,
                                  source_code='arithmetic')
  nan_codes = codes.clone()
  nan_codes[3, 5] = float('nan')
  with pytest.raises(ValueError):
    quantization.compute_RD_point(nan_codes, patches, dictionary, codebook,
                                  source_code='huffman', tables=tables)


def test_baseline_and_Mod1_slots(device, scene):
  """huff_tab1 is the list of scalar tables, huff_tab2 None; the test call
  reproduces compute_RD_point with those tables; codebooks without tables
  raise ValueError."""
  from utils import vector_quantization as quantization
  codes, patches, dictionary = (scene['codes'], scene['patches'],
                                scene['dictionary'])
  test_codes, test_patches = scene['test_codes'], scene['test_patches']

  out = twice(lambda: quantization.baseline_compute_RD_point(
      codes, patches, dictionary, quant_multiplier=MULT,
      binwidths=[WIDTH] * 64, source_code='huffman'))
  rate, dist, codebook, tab1, tab2 = out
  assert tab2 is None and isinstance(tab1, list) and len(tab1) == 64
  assert (rate, dist) == quantization.compute_RD_point(
      codes, patches, dictionary, codebook, source_code='huffman')[:2]
  assert rate == restated_rate(quantization.assign(codes, codebook), tab1,
                               scene['numel'])
  got = twice(lambda: quantization.baseline_compute_RD_point(
      test_codes, test_patches, dictionary, precomputed_codebook=codebook,
      precomputed_huff_tab1=tab1, precomputed_huff_tab2=tab2,
      source_code='huffman'))
  assert got == quantization.compute_RD_point(
      test_codes, test_patches, dictionary, codebook, source_code='huffman',
      tables=tab1)[:2]
  assert got[0] == restated_rate(quantization.assign(test_codes, codebook),
                                 tab1, scene['numel'])
  with pytest.raises(ValueError):
    quantization.baseline_compute_RD_point(
        test_codes, test_patches, dictionary, precomputed_codebook=codebook,
        source_code='huffman')
  with pytest.raises(ValueError):
    quantization.baseline_compute_RD_point(
        codes, patches, dictionary, quant_multiplier=MULT,
        binwidths=[WIDTH] * 64, source_code='jpeg')

  out = twice(lambda: quantization.Mod1_compute_RD_point(
      codes, patches, dictionary, quant_multiplier=MULT,
      init_binwidths=[WIDTH] * 64, max_iterations=vq_data.RD_ITERATIONS,
      epsilon=vq_data.RD_EPSILON, source_code='huffman')[:2])
  rate, dist, codebook, lengths, tab1 = quantization.Mod1_compute_RD_point(
      codes, patches, dictionary, quant_multiplier=MULT,
      init_binwidths=[WIDTH] * 64, max_iterations=vq_data.RD_ITERATIONS,
      epsilon=vq_data.RD_EPSILON, source_code='huffman')
  assert out == (rate, dist)
  assert isinstance(tab1, list) and len(tab1) == 64
  k = codebook['k'].cpu().numpy()
  assert [sorted(table) for table in tab1] == [list(range(kj)) for kj in k]
  train_indices = quantization.assign(codes, codebook, lengths, MULT)
  assert rate == restated_rate(train_indices, tab1, scene['numel'])
  got = twice(lambda: quantization.Mod1_compute_RD_point(
      test_codes, test_patches, dictionary, quant_multiplier=MULT,
      precomputed_codebook=codebook, precomputed_codebook_lengths=lengths,
      precomputed_huff_tab1=tab1, source_code='huffman'))
  assert got == quantization.compute_RD_point(
      test_codes, test_patches, dictionary, codebook, lengths=lengths,
      lagrange_mult=MULT, source_code='huffman', tables=tab1)[:2]
  assert got[0] == restated_rate(
      quantization.assign(test_codes, codebook, lengths, MULT), tab1,
      scene['numel'])
  with pytest.raises(ValueError):
    quantization.Mod1_compute_RD_point(
        test_codes, test_patches, dictionary, quant_multiplier=MULT,
        precomputed_codebook=codebook, precomputed_codebook_lengths=lengths,
        source_code='huffman')


@pytest.mark.parametrize('variant', [2, 3])
def test_Mod2_and_Mod3_slots(device, scene, variant):
  """huff_tab1 = the scalar tables, huff_tab2 = the vector table, huff_tab3
  None; the rate is that of the combined (b, 41 + 1) index array, scalars
  first; the test call reproduces compute_RD_point_mixed with those tables."""
  from utils import vector_quantization as quantization
  codes, patches, dictionary = (scene['codes'], scene['patches'],
                                scene['dictionary'])
  test_codes, test_patches = scene['test_codes'], scene['test_patches']
  scal, vec = vq_data.SCAL_CLUSTS, vq_data.VEC_CLUST
  entry = (quantization.Mod2_compute_RD_point if variant == 2
           else quantization.Mod3_compute_RD_point)
  vec_mult = 3000.0

  def train(source_code):
    return entry(codes, patches, dictionary, scal, vec,
                 scal_quant_multiplier=MULT, scal_binwidths=[WIDTH] * len(scal),
                 vec_quant_multiplier=vec_mult, vec_init_num_bins=100000,
                 max_iterations=vq_data.RD_ITERATIONS,
                 epsilon=vq_data.RD_EPSILON, source_code=source_code)
  out = train('huffman')
  assert twice(lambda: train('huffman')[:2]) == out[:2]
  rate, dist, scal_cbook, vec_cbook, vec_cw_len, tab1, tab2, tab3 = out
  assert tab3 is None and isinstance(tab1, list) and len(tab1) == len(scal)
  assert isinstance(tab2, dict)
  assert sorted(tab2) == list(range(int(vec_cbook['k'])))
  plain = train('entropy')
  assert plain[5:] == (None, None, None) and plain[1] == dist
  assert rate >= plain[0]

  mixed = {'vec_lengths': vec_cw_len, 'vec_lagrange_mult': vec_mult}
  scal_lengths, scal_mult = None, 0.0
  if variant == 3:
    scal_lengths, scal_mult = scal_cbook['lengths'], MULT
    mixed.update(scal_lengths=scal_lengths, scal_lagrange_mult=scal_mult)

  def combined(some_codes):
    at = torch.tensor(scal, device=device)
    first = quantization.assign(some_codes.index_select(1, at).contiguous(),
                                scal_cbook, scal_lengths, scal_mult)
    at = torch.tensor(vec, device=device)
    last = quantization.vector_assign(
        some_codes.index_select(1, at).contiguous(), vec_cbook, vec_cw_len,
        vec_mult)
    return torch.cat([first, last[:, None]], 1)
  assert rate == restated_rate(combined(codes), tab1 + [tab2], scene['numel'])

  def test_call(**tables):
    return entry(test_codes, test_patches, dictionary, scal, vec,
                 vec_quant_multiplier=vec_mult,
                 precomputed_scal_codebook=scal_cbook,
                 precomputed_vec_codebook=vec_cbook,
                 precomputed_vec_codebook_lengths=vec_cw_len,
                 source_code='huffman', **tables)
  got = twice(lambda: test_call(precomputed_huff_tab1=tab1,
                                precomputed_huff_tab2=tab2,
                                precomputed_huff_tab3=tab3))
  want = quantization.compute_RD_point_mixed(
      test_codes, test_patches, dictionary, scal, scal_cbook, vec, vec_cbook,
      source_code='huffman', tables=(tab1, tab2), **mixed)
  assert len(want) == 3 and got == want[:2]
  assert want[2] == (tab1, tab2)
  assert got[0] == restated_rate(combined(test_codes), tab1 + [tab2],
                                 scene['numel'])
  for tables in ({}, {'precomputed_huff_tab1': tab1},
                 {'precomputed_huff_tab2': tab2}):
    with pytest.raises(ValueError):
      test_call(**tables)
