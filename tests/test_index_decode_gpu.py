"""vtc_index_code_unpack (include/vtc_index_decode.h), the decoding half of
utils.index_coding and the from_stream rate-distortion points against the
restatement of tests/index_decode_data.py: integers and bytes, no tolerances.
Every device call runs twice and its bytes are compared.

The raw calls run behind guard bands (tests/fences.py) around `packed`,
`indices`, `row_bits`, `status` and a workspace of exactly the queried size;
the outputs are pre-filled with a pattern (0x5A) that is neither -1 nor a
valid index, so every element has to be written.

The shapes are those of the packer's tests (lane, wave and block edges, 1 to
4096 columns: below, at and above the 32 columns a wave collects) and one with
a kmax that is no power of two; the streams are built by data.image, not by the
product's packer, behind 0, 3 and 29 leading bits with gaps between the rows."""
import ctypes

import numpy as np
import pytest
import torch

import fences
import index_code_data as data
import index_decode_data as truth
import vq_data

pytestmark = pytest.mark.gpu

OK = 0
FILL = 0x5A


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


def raw_unpack(device, packed, offsets, tables, kmax, packed_bytes=None):
  """(indices, row_bits, status) as numpy arrays from one fenced call.
  `packed` holds at least one byte; packed_bytes (default: all of it) is what
  the call is told."""
  import vtc_hip
  from utils import index_coding
  lib = vtc_hip.load_library()
  packed = np.ascontiguousarray(packed, dtype=np.uint8)
  assert packed.size >= 1
  if packed_bytes is None:
    packed_bytes = packed.size
  assert 0 <= packed_bytes <= packed.size
  offsets = np.ascontiguousarray(offsets, dtype=np.int64)
  b, m = len(offsets) - 1, len(tables)
  code, length = index_coding.index_table_arrays(tables, kmax)
  code, length = dev(code.view(np.int64), device), dev(length, device)
  f = {}
  # the payload is exactly the bytes the call may read
  bits_from, f['packed'] = fences.fenced_copy(
      packed[:max(packed_bytes, 1)], device)
  starts, f['offsets'] = fences.fenced_copy(offsets, device)
  indices, f['indices'] = fences.fenced((b, m), torch.int32, device, fill=FILL)
  rows, f['row_bits'] = fences.fenced((b,), torch.int32, device, fill=FILL)
  status, f['status'] = fences.fenced((3,), torch.int64, device, fill=FILL)
  need = lib.vtc_index_code_unpack_workspace_bytes(m, kmax)
  assert need > 0
  ws, f['workspace'] = fences.fenced_workspace(need, device)
  rc = lib.vtc_index_code_unpack(
      p(bits_from), packed_bytes, p(starts), b, m, p(code), p(length), kmax,
      p(indices), p(rows), p(status), p(ws), need,
      vtc_hip.current_stream(device))
  torch.cuda.synchronize(device)
  assert rc == OK, lib.vtc_last_error()
  for name, fence in f.items():
    fence.assert_intact(name)
  assert np.array_equal(starts.cpu().numpy(), offsets)
  return indices.cpu().numpy(), rows.cpu().numpy(), status.cpu().numpy()


def check_against_restatement(device, packed, offsets, tables, kmax,
                              packed_bytes=None):
  """The device's answer is the restatement's; returns (indices, row_bits,
  malformed rows, bad position) of the restatement."""
  got = twice(lambda: raw_unpack(device, packed, offsets, tables, kmax,
                                 packed_bytes))
  seen = np.asarray(packed, np.uint8)[:len(packed) if packed_bytes is None
                                      else packed_bytes]
  indices, rows, malformed, bad = truth.decode(seen, offsets, tables, kmax)
  assert got[2].tolist() == truth.status(malformed, bad)
  assert np.array_equal(got[0], indices) and got[0].dtype == np.int32
  assert np.array_equal(got[1], rows) and got[1].dtype == np.int32
  return indices, rows, malformed, bad


# ------------------------------------------------------------ exact decoding
@pytest.mark.parametrize('shape', truth.SHAPES, ids=truth.IDS)
def test_streams_of_the_restatement_decode(device, shape):
  tables, _ = data.case_tables(*shape)
  host = data.case_indices(*shape)
  want_rows = data.row_bits(host, tables)
  for lead in data.LEADS:
    packed, offsets = truth.case_stream(shape, lead)
    indices, rows, status = twice(lambda: raw_unpack(
        device, packed, offsets, tables, shape[2]))
    assert status.tolist() == [0, 0, 0]
    assert np.array_equal(indices, host)
    assert np.array_equal(rows, want_rows)
    # what the caller compares: the gaps are what the rows left unread
    assert np.array_equal(np.diff(offsets) - rows, data.gaps(shape[0]))


@pytest.mark.parametrize('shape', truth.SHAPES, ids=truth.IDS)
def test_round_trip_through_the_product(device, shape):
  from utils import index_coding
  tables, _ = data.case_tables(*shape)
  indices = dev(data.case_indices(*shape), device)
  packed, offsets = index_coding.pack_index_streams(indices, tables)
  back = twice(lambda: index_coding.unpack_index_streams(packed, offsets,
                                                         tables))
  assert back.dtype == torch.int32 and torch.equal(back, indices)


@pytest.mark.parametrize('flipped', [False, True], ids=['zeros', 'ones'])
def test_every_length_from_1_to_64(device, flipped):
  """m = 1, the 65-symbol table, one row per symbol: every length is read,
  among them exactly K and K + 1 bits (the lookup's edge), 57 (where the bit
  window needs its extra byte) and 64; the long codewords are runs of zeros
  in the table and of ones in its complement."""
  table = truth.long_table()
  if flipped:
    table = data.complement(table)
  host = np.arange(65, dtype=np.int32)[:, None]
  bits = data.row_bits(host, [table])
  assert sorted(bits.tolist()) == list(range(1, 65)) + [64]
  for lead in data.LEADS:
    offsets = data.layout(bits, lead, data.gaps(65))
    nbytes = -(-int(offsets[-1]) // 8)
    packed, dropped = data.image(host, [table], offsets, nbytes)
    assert dropped == 0
    indices, rows, malformed, bad = check_against_restatement(
        device, packed, offsets, [table], 65)
    assert malformed == [] and bad is None
    assert np.array_equal(indices, host) and np.array_equal(rows, bits)


def test_empty_codewords(device):
  """A one-symbol column costs nothing: alone (no stream bits at all, and a
  call told of 0 bytes), and on either side of columns 63 / 64."""
  one, two = {0: ''}, {0: '0', 1: '1'}
  b = 70
  offsets = np.zeros(b + 1, np.int64)
  for packed_bytes in (0, 1):
    indices, rows, malformed, bad = check_against_restatement(
        device, np.array([0xFF], np.uint8), offsets, [one], 1, packed_bytes)
    assert (indices == 0).all() and (rows == 0).all() and malformed == []

  rs = np.random.RandomState(5)
  for at in (63, 64):
    tables = [two] * 66
    tables[at] = one
    host = rs.randint(0, 2, size=(b, 66)).astype(np.int32)
    host[:, at] = 0
    bits = data.row_bits(host, tables)
    assert (bits == 65).all()
    offsets = data.layout(bits, 3, data.gaps(b))
    nbytes = -(-int(offsets[-1]) // 8)
    packed, _ = data.image(host, tables, offsets, nbytes)
    indices, rows, malformed, bad = check_against_restatement(
        device, packed, offsets, tables, 2)
    assert np.array_equal(indices, host) and malformed == []


# ---------------------------------------------------------- malformed inputs
SHAPE = (5, 23, 64)


def _case(lead=3):
  tables, _ = data.case_tables(*SHAPE)
  packed, offsets = truth.case_stream(SHAPE, lead)
  return tables, data.case_indices(*SHAPE), packed, offsets.copy()


def test_buffer_one_byte_short(device):
  tables, host, packed, offsets = _case()
  indices, rows, malformed, bad = check_against_restatement(
      device, packed, offsets, tables, SHAPE[2], len(packed) - 1)
  assert malformed == [4] and np.array_equal(indices[:4], host[:4])
  assert -1 in indices[4]


def test_row_end_one_bit_early(device):
  """offsets[b] one bit early under the non-empty last codeword of the last
  row: that codeword would pass the row's end."""
  tables, host, packed, offsets = _case()
  assert len(tables[-1][int(host[-1, -1])]) > 0 and data.gaps(5)[-1] == 0
  offsets[-1] -= 1
  indices, rows, malformed, bad = check_against_restatement(
      device, packed, offsets, tables, SHAPE[2])
  assert malformed == [4] and np.array_equal(indices[:4], host[:4])
  assert np.array_equal(indices[4, :-1], host[4, :-1]) and indices[4, -1] == -1


def test_decreasing_and_negative_offsets(device):
  tables, host, packed, offsets = _case()
  offsets[2] = offsets[3] + 1       # row 1 ends later, row 2 starts past its end
  indices, rows, malformed, bad = check_against_restatement(
      device, packed, offsets, tables, SHAPE[2])
  assert malformed == [2] and (indices[2] == -1).all() and rows[2] == 0
  assert np.array_equal(indices[[0, 1, 3, 4]], host[[0, 1, 3, 4]])

  tables, host, packed, offsets = _case()
  offsets[0] = -1
  indices, rows, malformed, bad = check_against_restatement(
      device, packed, offsets, tables, SHAPE[2])
  assert malformed == [0] and (indices[0] == -1).all()
  assert np.array_equal(indices[1:], host[1:])      # the rows behind decode


def test_offset_beyond_the_buffer(device):
  tables, host, packed, offsets = _case()
  offsets[4] = 8 * len(packed) + 5
  offsets[5] = 8 * len(packed) + 400
  indices, rows, malformed, bad = check_against_restatement(
      device, packed, offsets, tables, SHAPE[2])
  assert malformed == [4] and (indices[4] == -1).all() and rows[4] == 0
  assert np.array_equal(indices[:4], host[:4])


def test_no_codeword_matches(device):
  """'11' under the incomplete table {'00', '01', '10'}; a column without any
  codeword.  The rows behind a malformed one still decode."""
  partial = [{0: '00', 1: '01', 2: '10'}]
  indices, rows, malformed, bad = check_against_restatement(
      device, np.array([0b00111000], np.uint8), np.array([0, 2, 4, 6]),
      partial, 3)
  assert indices.tolist() == [[0], [-1], [2]] and rows.tolist() == [2, 0, 2]

  two = {0: '0', 1: '1'}
  indices, rows, malformed, bad = check_against_restatement(
      device, np.array([0b01100000], np.uint8), np.array([0, 2, 4]),
      [two, {}, two], 2)
  assert indices.tolist() == [[0, -1, -1], [1, -1, -1]]
  assert malformed == [0, 1] and rows.tolist() == [1, 1]


@pytest.mark.parametrize('name,table,symbol', [
    ('equal', {0: '0', 1: '10', 2: '10'}, 1),
    ('prefix', {0: '00', 1: '1', 2: '10'}, 1),
    ('empty', {0: '', 1: '0'}, 0)])
def test_bad_tables(device, name, table, symbol):
  """The first flat position is reported and nothing is decoded; through
  Python the same tables raise before any device work."""
  from utils import index_coding
  good, kmax = {0: '0', 1: '10', 2: '11'}, 4
  tables = [good, table, good]
  offsets = np.array([0, 3, 6, 9], np.int64)
  indices, rows, malformed, bad = check_against_restatement(
      device, np.array([0x12, 0x34], np.uint8), offsets, tables, kmax)
  assert bad == kmax + symbol
  assert (indices == -1).all() and (rows == 0).all()
  with pytest.raises(ValueError):
    # CPU tensors: reaching the device checks would raise VtcHipError instead
    index_coding.unpack_index_streams(torch.zeros(2, dtype=torch.uint8),
                                      torch.from_numpy(offsets), tables)


# -------------------------------------------------------------- Python layer
def test_python_reports_malformed_and_loose_rows(device):
  from utils import index_coding
  tables, host, packed, offsets = _case()
  on = lambda a: dev(a, device)
  with pytest.raises(ValueError, match='do not use up'):   # data.gaps
    index_coding.unpack_index_streams(on(packed), on(offsets), tables)
  back = index_coding.unpack_index_streams(on(packed), on(offsets), tables,
                                           exact=False)
  assert np.array_equal(back.cpu().numpy(), host)
  with pytest.raises(ValueError,
                     match='1 malformed rows of 5, the first is row 4'):
    index_coding.unpack_index_streams(on(packed[:-1]), on(offsets), tables,
                                      exact=False)
  offsets[-1] -= 1
  with pytest.raises(ValueError, match='row 4, undecoded from column 22 on'):
    index_coding.unpack_index_streams(on(packed), on(offsets), tables,
                                      exact=False)


def test_parse_index_stream(device):
  from utils import index_coding
  for shape in ((5, 23, 64), (3, 65, 8), (63, 1, 4096)):
    tables, _ = data.case_tables(*shape)
    for row in data.case_indices(*shape)[:3]:
      text = data.stream(row, tables)
      assert index_coding.parse_index_stream(text, tables) == row.tolist()
  assert index_coding.parse_index_stream('', [{0: ''}, {0: ''}]) == [0, 0]
  with pytest.raises(ValueError):
    index_coding.parse_index_stream('0', [{0: '0', 1: '1'}] * 2)
  with pytest.raises(ValueError):                   # a bit too many
    index_coding.parse_index_stream('010', [{0: '0', 1: '1'}] * 2)


WIDTH, MULT = 5.0, 2.0


@pytest.fixture(scope='module')
def scene(device):
  s = vq_data.scene()
  return {k: dev(s[k], device) for k in ('codes', 'patches', 'dictionary')}


def test_decode_codes(device, scene):
  from utils import index_coding
  from utils import quantization
  codes = scene['codes']
  codebook = quantization._uniform_for(codes, [WIDTH] * 64, MULT)
  indices, dequantized = quantization.assign(codes, codebook,
                                             return_dequantized=True)
  tables = index_coding.index_huffman_tables(
      quantization.index_counts(indices, codebook[0].shape[1]), codebook[1])
  packed, offsets = index_coding.pack_index_streams(indices, tables)
  got = twice(lambda: quantization.decode_codes(packed, offsets, tables,
                                                codebook))
  assert got.dtype == torch.float32
  assert torch.equal(got, quantization.dequantize_assignments(indices,
                                                              codebook))
  assert torch.equal(got, dequantized)


def test_decode_codes_mixed(device, scene):
  from utils import index_coding
  from utils import vector_quantization as vq
  codes = scene['codes']
  # the clusters leave columns 0 and 4 to neither part
  scal, vec = vq_data.SCAL_CLUSTS[:7], vq_data.VEC_CLUST[2:9]
  at = lambda cluster: torch.tensor(cluster, device=device)
  scal_codes = codes.index_select(1, at(scal)).contiguous()
  vec_codes = codes.index_select(1, at(vec)).contiguous()
  scal_book = vq._scalar._uniform_for(scal_codes, [WIDTH] * len(scal), MULT)
  vec_book = vq.initial_vector_codebook(vec_codes, 16)
  first = vq.assign(scal_codes, scal_book)
  last = vq.vector_assign(vec_codes, vec_book)
  tables = index_coding.index_huffman_tables(
      vq.index_counts(first, scal_book[0].shape[1]), scal_book[1])
  tables += index_coding.index_huffman_tables(
      vq.vector_index_counts(last, vec_book.shape[0]))
  packed, offsets = index_coding.pack_index_streams(
      torch.cat([first, last[:, None]], 1), tables)
  got = twice(lambda: vq.decode_codes_mixed(packed, offsets, tables, scal,
                                            scal_book, vec, vec_book, 64))
  want = torch.zeros_like(codes)
  want.index_copy_(1, at(scal), vq.dequantize_assignments(first, scal_book))
  want.index_copy_(1, at(vec), vq.vector_dequantize(last, vec_book))
  assert torch.equal(got, want) and got.shape == (codes.shape[0], 64)
  assert not got[:, [0, 4]].any() and got.any()
  with pytest.raises(ValueError):
    vq.decode_codes_mixed(packed, offsets, tables[:-1], scal, scal_book, vec,
                          vec_book, 64)


def test_rd_points_from_the_stream(device, scene):
  """from_stream=True returns exactly the rate and distortion of the default
  path; the four entries forward the keyword; any other source code raises."""
  from utils import vector_quantization as vq
  codes, patches, dictionary = (scene['codes'], scene['patches'],
                                scene['dictionary'])
  codebook = vq._scalar._uniform_for(codes, [WIDTH] * 64, MULT)
  plain = vq.compute_RD_point(codes, patches, dictionary, codebook,
                              source_code='huffman')
  got = twice(lambda: vq.compute_RD_point(
      codes, patches, dictionary, codebook, source_code='huffman',
      from_stream=True))
  assert got == plain and got[0] > 0
  got = vq.compute_RD_point(codes, patches, dictionary, codebook,
                            source_code='huffman', tables=plain[2],
                            from_stream=True)
  assert got[:2] == plain[:2] and got[2] is plain[2]

  scal, vec = vq_data.SCAL_CLUSTS, vq_data.VEC_CLUST
  scal_book = vq._scalar._uniform_for(
      codes.index_select(1, torch.tensor(scal, device=device)).contiguous(),
      [WIDTH] * len(scal), MULT)
  vec_book = vq.initial_vector_codebook(
      codes.index_select(1, torch.tensor(vec, device=device)).contiguous(), 16)
  mixed = lambda **kw: vq.compute_RD_point_mixed(
      codes, patches, dictionary, scal, scal_book, vec, vec_book,
      source_code='huffman', **kw)
  assert twice(lambda: mixed(from_stream=True)) == mixed()

  common = dict(max_iterations=vq_data.RD_ITERATIONS,
                epsilon=vq_data.RD_EPSILON)
  entries = [
      lambda **kw: vq.baseline_compute_RD_point(
          codes, patches, dictionary, quant_multiplier=MULT,
          binwidths=[WIDTH] * 64, **kw),
      lambda **kw: vq.Mod1_compute_RD_point(
          codes, patches, dictionary, quant_multiplier=MULT,
          init_binwidths=[WIDTH] * 64, **common, **kw)]
  for entry in (vq.Mod2_compute_RD_point, vq.Mod3_compute_RD_point):
    entries.append(lambda entry=entry, **kw: entry(
        codes, patches, dictionary, scal, vec, scal_quant_multiplier=MULT,
        scal_binwidths=[WIDTH] * len(scal), vec_quant_multiplier=3000.0,
        vec_init_num_bins=100000, **common, **kw))
  for entry in entries:
    assert (entry(source_code='huffman', from_stream=True)[:2] ==
            entry(source_code='huffman')[:2])
    with pytest.raises(ValueError, match='from_stream'):
      entry(source_code='entropy', from_stream=True)
    with pytest.raises(ValueError, match='from_stream'):
      entry(from_stream=True)                      # 'entropy' is the default
  for source_code in ('entropy', 'jpeg'):
    with pytest.raises(ValueError, match='from_stream'):
      vq.compute_RD_point(codes, patches, dictionary, codebook,
                          source_code=source_code, from_stream=True)
  with pytest.raises(ValueError, match='from_stream'):
    vq.compute_RD_point_mixed(codes, patches, dictionary, scal, scal_book,
                              vec, vec_book, from_stream=True)
