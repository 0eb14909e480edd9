"""vtc_index_ans_split_sizes / _pack / _unpack
(include/ext/vtc_index_ans_split.h) and their Python interface against the
restatement of tests/index_ans_split_data.py, byte for byte and index for
index, every call twice; then source_code='ans_split' of the mixed
rate-distortion entries on codebooks of more than 4096 codewords.  All
comparisons are between integers or bytes.

The raw calls run with outputs pre-filled with a pattern the call has to
overwrite and with a 0xFF-filled workspace of exactly the queried size."""
import numpy as np
import pytest
import torch

import index_ans_data as one_table
import index_ans_split_data as truth
import vq_data
import vq_large_data
from test_index_ans_gpu import dev, p, twice, scene  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

OK = 0
LEADS = (0, 3)
LARGE = vq_large_data.MAX_CODEWORDS
WIDTH, MULT, ROWS = 5.0, 2.0, 100


def device_freq(freq, device):
  return dev(np.ascontiguousarray(freq).view(np.int16), device)


def _workspace(lib, kmax, device):
  need = lib.vtc_index_ans_split_workspace_bytes(kmax)
  assert need > 0
  return torch.full((need,), 0xFF, dtype=torch.uint8, device=device)


class Coder(object):
  """The three raw calls on one pair of tables."""

  def __init__(self, device, freq_hi, freq_lo, kmax, rows):
    import vtc_hip
    self.hip, self.lib = vtc_hip, vtc_hip.load_library()
    self.device, self.kmax, self.rows = device, kmax, rows
    self.host = (freq_hi, freq_lo)
    self.freq_hi = device_freq(freq_hi, device)
    self.freq_lo = device_freq(freq_lo, device)

  def sizes(self, indices):
    """(stream_bytes, status) as numpy arrays."""
    b = indices.shape[0]
    n = truth.streams_of(b, self.rows)
    sizes = torch.full((n,), -7, dtype=torch.int32, device=self.device)
    status = torch.full((3,), -7, dtype=torch.int64, device=self.device)
    ws = _workspace(self.lib, self.kmax, self.device)
    rc = self.lib.vtc_index_ans_split_sizes(
        p(indices), b, p(self.freq_hi), p(self.freq_lo), self.kmax, self.rows,
        p(sizes), p(status), p(ws), ws.numel(),
        self.hip.current_stream(self.device))
    assert rc == OK, self.lib.vtc_last_error()
    return sizes.cpu().numpy(), status.cpu().numpy()

  def pack(self, indices, sizes, offsets, nbytes, spare=64):
    """(packed [nbytes], status) as numpy arrays; `packed` pre-filled with
    ones and followed by `spare` bytes that must keep them."""
    packed = torch.full((nbytes + spare,), 0xFF, dtype=torch.uint8,
                        device=self.device)
    status = torch.full((3,), -7, dtype=torch.int64, device=self.device)
    ws = _workspace(self.lib, self.kmax, self.device)
    sizes = dev(np.asarray(sizes, np.int32), self.device)
    offsets = dev(np.asarray(offsets, np.int64), self.device)
    rc = self.lib.vtc_index_ans_split_pack(
        p(indices), indices.shape[0], p(self.freq_hi), p(self.freq_lo),
        self.kmax, self.rows, p(sizes), p(offsets), p(packed), nbytes,
        p(status), p(ws), ws.numel(), self.hip.current_stream(self.device))
    assert rc == OK, self.lib.vtc_last_error()
    host = packed.cpu().numpy()
    assert (host[nbytes:] == 0xFF).all(), 'a store landed past packed_bytes'
    return host[:nbytes], status.cpu().numpy()

  def unpack(self, packed, offsets, b):
    """(indices, used_bytes, status) as numpy arrays."""
    n = truth.streams_of(b, self.rows)
    packed = dev(np.asarray(packed, np.uint8), self.device)
    indices = torch.full((b,), -7, dtype=torch.int32, device=self.device)
    used = torch.full((n,), -7, dtype=torch.int32, device=self.device)
    status = torch.full((3,), -7, dtype=torch.int64, device=self.device)
    ws = _workspace(self.lib, self.kmax, self.device)
    offsets = dev(np.asarray(offsets, np.int64), self.device)
    rc = self.lib.vtc_index_ans_split_unpack(
        p(packed if packed.numel() else ws), packed.numel(), p(offsets), b,
        p(self.freq_hi), p(self.freq_lo), self.kmax, self.rows, p(indices),
        p(used), p(status), p(ws), ws.numel(),
        self.hip.current_stream(self.device))
    assert rc == OK, self.lib.vtc_last_error()
    return indices.cpu().numpy(), used.cpu().numpy(), status.cpu().numpy()

  def decodes_as_restated(self, packed, offsets, b):
    want = truth.decode(packed, offsets, b, *self.host, self.kmax, self.rows)
    got, used, status = twice(lambda: self.unpack(packed, offsets, b))
    assert status.tolist() == want[2]
    assert np.array_equal(got, want[0]) and np.array_equal(used, want[1])
    return want


def _exact(device, host, freq_hi, freq_lo, kmax, rows, streams):
  """Sizes, packed bytes behind 0 and 3 leading bytes with gaps, and the way
  back, against the restated streams."""
  b, n = len(host), len(streams)
  want_sizes = np.array([len(s) for s in streams], np.int32)
  coder = Coder(device, freq_hi, freq_lo, kmax, rows)
  indices = dev(host, device)
  sizes, status = twice(lambda: coder.sizes(indices))
  assert np.array_equal(sizes, want_sizes) and sizes.dtype == np.int32
  assert status.tolist() == [0, 0, 0]
  for lead in LEADS:
    offsets = truth.layout(want_sizes, lead, truth.gaps(n))
    nbytes = int(offsets[-1])
    want, skipped = truth.image(streams, offsets, nbytes)
    assert skipped == 0
    packed, status = twice(lambda: coder.pack(indices, want_sizes, offsets,
                                              nbytes))
    assert status.tolist() == [0, 0, 0]
    # every stream in its place, every byte outside the streams zero
    assert np.array_equal(packed, want), lead
    got, used, status = twice(lambda: coder.unpack(want, offsets, b))
    assert status.tolist() == [0, 0, 0]
    assert np.array_equal(got, host) and np.array_equal(used, want_sizes)
  return want_sizes


# ------------------------------------------------------------ exact streams
@pytest.mark.parametrize('case', truth.CASES, ids=truth.IDS)
def test_sizes_streams_and_the_way_back(device, case):
  from utils import index_coding
  b, kmax, rows = case
  host = truth.case_indices(*case)
  freq_hi, freq_lo = truth.case_tables(*case)
  streams = truth.case_streams(*case)
  want_sizes = _exact(device, host, freq_hi, freq_lo, kmax, rows, streams)
  n = len(streams)

  # the Python interface: byte offsets from jpeg.bit_offsets, no gaps
  indices, tables = dev(host, device), (freq_hi, freq_lo)
  got_sizes = twice(lambda: index_coding.index_ans_split_stream_bytes(
      indices, tables, rows))
  assert got_sizes.dtype == torch.int32
  assert np.array_equal(got_sizes.cpu().numpy(), want_sizes)
  packed, offsets, got_rows = twice(
      lambda: index_coding.pack_index_ans_split(indices, tables, rows))
  assert got_rows == rows
  assert packed.dtype == torch.uint8 and offsets.dtype == torch.int64
  assert np.array_equal(offsets.cpu().numpy(),
                        truth.layout(want_sizes, 0, [0] * n))
  assert packed.cpu().numpy().tobytes() == b''.join(streams)
  back = twice(lambda: index_coding.unpack_index_ans_split(
      packed, offsets, tables, b, rows))
  assert back.dtype == torch.int32 and back.shape == (b,)
  assert np.array_equal(back.cpu().numpy(), host)


@pytest.mark.parametrize('name', sorted(truth.hand_tables()))
def test_hand_made_tables(device, name):
  freq_hi, freq_lo, kmax, host = truth.hand_tables()[name]
  assert truth.bad_table(freq_hi, freq_lo, kmax) == 0     # classified first
  for rows in (64, 1000):
    streams, status = truth.encode(host, freq_hi, freq_lo, kmax, rows)
    assert status == [0, 0, 0]
    sizes = _exact(device, host, freq_hi, freq_lo, kmax, rows, streams)
    if name == 'single':
      assert set(sizes.tolist()) == {truth.HEADER}


def test_the_default_rows_per_stream(device):
  from utils import index_coding
  case = (300, 5000, 100)
  host, tables = truth.case_indices(*case), truth.case_tables(*case)
  indices = dev(host, device)
  packed, offsets, rows = index_coding.pack_index_ans_split(indices, tables)
  assert rows == 65536 and offsets.shape[0] == 2
  # the Python interface hands the calls kmax = 256 H: the same streams
  top = len(tables[0])
  streams, _ = truth.encode(host, *tables, truth.LO * top, rows)
  assert streams == truth.encode(host, *tables, 5000, rows)[0]
  assert packed.cpu().numpy().tobytes() == b''.join(streams)
  back = index_coding.unpack_index_ans_split(packed, offsets, tables, 300,
                                             None)
  assert np.array_equal(back.cpu().numpy(), host)
  # bytes left over in a slot are reported, and refused only on request
  longer = torch.cat([packed, torch.zeros(6, dtype=torch.uint8,
                                          device=device)])
  wide = offsets + torch.tensor([0, 6], device=device)
  with pytest.raises(ValueError, match='do not use up'):
    index_coding.unpack_index_ans_split(longer, wide, tables, 300, rows)
  back = index_coding.unpack_index_ans_split(longer, wide, tables, 300, rows,
                                             exact=False)
  assert np.array_equal(back.cpu().numpy(), host)
  with pytest.raises(ValueError, match='malformed'):
    index_coding.unpack_index_ans_split(packed[:-2].contiguous(),
                                        offsets - torch.tensor(
                                            [0, 2], device=device),
                                        tables, 300, rows)
  with pytest.raises(ValueError):
    index_coding.pack_index_ans_split(indices, tables, (1 << 24) + 1)
  wrong = (tables[0].copy(), tables[1])
  wrong[0][0] += 1
  with pytest.raises(ValueError, match='hi frequencies sum to'):
    index_coding.pack_index_ans_split(indices, wrong)
  wrong = (tables[0], tables[1].copy())
  wrong[1][3, 0] += 1
  with pytest.raises(ValueError, match='row 3 sum to'):
    index_coding.unpack_index_ans_split(packed, offsets, wrong, 300, rows)
  with pytest.raises(NotImplementedError, match='at most 131072'):
    index_coding.pack_index_ans_split(
        indices, (np.zeros(513, np.uint16), np.zeros((513, 256), np.uint16)))


# ------------------------------------------------------------ bounded stores
def test_a_buffer_one_byte_short(device):
  """The last stream does not fit: it is skipped whole and counted, and
  nothing lands outside."""
  case = (300, 131072, 100)
  b, kmax, rows = case
  streams = truth.case_streams(*case)
  sizes = np.array([len(s) for s in streams], np.int32)
  offsets = truth.layout(sizes, 3, truth.gaps(3)[:2] + [0])
  nbytes = int(offsets[-1]) - 1
  want, skipped = truth.image(streams, offsets, nbytes)
  assert skipped == 1 and (want[offsets[2]:] == 0).all()
  coder = Coder(device, *truth.case_tables(*case), kmax, rows)
  indices = dev(truth.case_indices(*case), device)
  packed, status = twice(lambda: coder.pack(indices, sizes, offsets, nbytes))
  assert status.tolist() == [0, 0, 1]
  assert np.array_equal(packed, want)


def test_slots_and_sizes_that_are_not_the_coders(device):
  """A slot that overlaps the next, a negative offset, a size below the 256
  bytes of states and an odd one skip the stream before any store; a size two
  bytes short of the coder's own is counted, written inside its slot only,
  and leaves the neighbours intact."""
  case = (300, 131072, 100)
  b, kmax, _ = case
  rows = 45                    # 7 streams
  tables = truth.case_tables(*case)
  # uniform over all symbols: 17 bits an index, every lane emits at once
  host = np.random.RandomState(4).randint(0, kmax, size=b).astype(np.int32)
  streams, _ = truth.encode(host, *tables, kmax, rows)
  n = len(streams)
  assert n == 7
  own = np.array([len(s) for s in streams], np.int32)
  assert own.min() > truth.HEADER + 40
  offsets = truth.layout(own, 5, [0] * n)
  coder = Coder(device, *tables, kmax, rows)
  indices = dev(host, device)
  nbytes = int(offsets[-1])

  sizes = own.copy()
  sizes[1] += 2          # passes offsets[2]
  sizes[2] = 254         # no room for the states
  sizes[3] -= 1          # odd
  sizes[5] -= 2          # one word short: counted, contents unspecified
  skipped = [1, 2, 3]
  packed, status = twice(lambda: coder.pack(indices, sizes, offsets, nbytes))
  assert status.tolist() == [0, 0, 4]
  kept = [s if i not in skipped + [5] else b'\0' * len(s)
          for i, s in enumerate(streams)]
  want, _ = truth.image(kept, offsets, nbytes)
  outside_5 = np.ones(nbytes, bool)
  outside_5[offsets[5]:offsets[5] + sizes[5]] = False
  assert np.array_equal(packed[outside_5], want[outside_5])

  moved = offsets.copy()
  moved[0] = -1
  packed, status = coder.pack(indices, own, moved, nbytes)
  assert status.tolist() == [0, 0, 1]
  want, _ = truth.image([b'\0' * len(streams[0])] + streams[1:], offsets,
                        nbytes)
  assert np.array_equal(packed, want)


# ---------------------------------------------------------- uncodable entries
def test_uncodable_entries(device):
  """All four kinds: negative, >= kmax, freq_hi[hi] = 0, freq_lo[hi, lo] =
  0."""
  from utils import index_coding
  freq_hi, freq_lo, kmax, host = truth.hand_tables()['hi-gap']
  freq_lo = freq_lo.copy()
  freq_lo[2, 9] += freq_lo[2, 8]       # lo 8 of block 2 is absent
  freq_lo[2, 8] = 0
  host = np.where(host == 2 * truth.LO + 8, 0, host).astype(np.int32)
  rows = 64
  host[70] = -1                        # the index of a NaN code
  host[71] = kmax                      # past the table
  host[130] = truth.LO + 5             # a hi symbol of frequency 0
  host[199] = 2 * truth.LO + 8         # a lo symbol of frequency 0
  streams, want_status = truth.encode(host, freq_hi, freq_lo, kmax, rows)
  assert want_status == [4, 1 + 70, 0]
  want_sizes = np.array([len(s) for s in streams], np.int32)
  coder = Coder(device, freq_hi, freq_lo, kmax, rows)
  indices = dev(host, device)
  sizes, status = twice(lambda: coder.sizes(indices))
  assert status.tolist() == want_status
  assert np.array_equal(sizes, want_sizes)
  offsets = truth.layout(want_sizes, 0, [0] * len(streams))
  packed, status = twice(lambda: coder.pack(indices, want_sizes, offsets,
                                            int(offsets[-1])))
  assert status.tolist() == want_status
  assert packed.tobytes() == b''.join(streams)
  with pytest.raises(KeyError, match=r'no frequency for index -1 \(row 70\)'):
    index_coding.index_ans_split_stream_bytes(indices, (freq_hi, freq_lo),
                                              rows)
  with pytest.raises(KeyError, match='4 such entries'):
    index_coding.pack_index_ans_split(indices, (freq_hi, freq_lo), rows)
  # only the later ones: the first row moves
  host[70], host[71] = 0, 0
  _, want_status = truth.encode(host, freq_hi, freq_lo, kmax, rows)
  assert want_status == [2, 1 + 130, 0]
  _, status = coder.sizes(dev(host, device))
  assert status.tolist() == want_status


# ------------------------------------------------------- decoder robustness
@pytest.fixture(scope='module')
def three_streams():
  case = (300, 131072, 100)
  host, tables = truth.case_indices(*case), truth.case_tables(*case)
  streams = truth.case_streams(*case)
  sizes = [len(s) for s in streams]
  offsets = truth.layout(sizes, 0, [0, 0, 0])
  packed, _ = truth.image(streams, offsets, int(offsets[-1]))
  return case, host, tables, packed, offsets


def test_a_slot_cut_by_two_bytes(device, three_streams):
  (b, kmax, rows), host, tables, packed, offsets = three_streams
  coder = Coder(device, *tables, kmax, rows)
  shifted = np.concatenate([packed[:offsets[2] - 2], packed[offsets[2]:]])
  moved = np.array([offsets[0], offsets[1], offsets[2] - 2, offsets[3] - 2])
  got, used, status = coder.decodes_as_restated(shifted, moved, b)
  assert status == [1, 2, 0]                   # the restatement, first
  assert np.array_equal(got[:100], host[:100])
  assert np.array_equal(got[200:], host[200:])
  assert (got[100:200] == -1).any() and used[1] <= moved[2] - moved[1]


def test_one_flipped_word(device, three_streams):
  """Everything decodes to something and, as a rule, the end states tell.  Not
  always: where neighbouring symbols share a frequency, a flipped slot bit
  picks the neighbour at the same place within it and the state goes on as it
  was.  The restatement says which flip is which; the device follows it in
  both."""
  (b, kmax, rows), host, tables, packed, offsets = three_streams
  coder = Coder(device, *tables, kmax, rows)
  seen = {}
  for at in range(truth.HEADER, truth.HEADER + 60):
    flipped = packed.copy()
    flipped[offsets[1] + at] ^= 0x40
    _, _, status = truth.decode(flipped, offsets, b, *tables, kmax, rows)
    seen.setdefault(status[0], flipped)
  assert status[2] == 0 and 1 in seen
  for malformed, flipped in sorted(seen.items()):
    got, used, status = coder.decodes_as_restated(flipped, offsets, b)
    assert status[:2] == ([1, 2] if malformed else [0, 0])
    assert ((got >= -1) & (got < kmax)).all()   # -1: it may run dry
    assert np.array_equal(got[:100], host[:100])
    assert np.array_equal(got[200:], host[200:])


def test_offsets_that_decrease_and_short_buffers(device, three_streams):
  (b, kmax, rows), host, tables, packed, offsets = three_streams
  coder = Coder(device, *tables, kmax, rows)
  wrong = offsets.copy()
  wrong[1] = offsets[2] + 4
  got, used, status = coder.decodes_as_restated(packed, wrong, b)
  assert status[0] >= 1 and (got[100:200] == -1).all() and used[1] == 0
  wrong = offsets.copy()
  wrong[0] = -2
  got, used, status = coder.decodes_as_restated(packed, wrong, b)
  assert status == [1, 1, 0] and (got[:100] == -1).all()
  # the buffer ends inside the states of the last stream
  got, used, status = coder.decodes_as_restated(
      packed[:offsets[2] + 100], offsets, b)
  assert status == [1, 3, 0] and (got[200:] == -1).all() and used[2] == 0
  assert np.array_equal(got[:200], host[:200])
  # no bytes at all
  got, used, status = coder.decodes_as_restated(packed[:0], offsets, b)
  assert status == [3, 1, 0] and (got == -1).all() and (used == 0).all()


def test_bad_tables(device, three_streams):
  """A bad hi sum, a bad lo row, a nonzero entry past kmax: nothing is coded
  or decoded, by any of the three calls."""
  (b, _, rows), host, _, _, _ = three_streams
  freq_hi, freq_lo, kmax, _ = truth.hand_tables()['partial']
  host = np.minimum(host, kmax - 1)
  hi_sum = freq_hi.copy()
  hi_sum[0] += 1
  lo_row = freq_lo.copy()
  lo_row[3, 0] += 1
  lo_row[1, 9] -= 1
  past = freq_lo.copy()
  past[4, 4] -= 1
  past[4, 5] += 1                # index 256 * 4 + 5 = kmax
  offsets = truth.layout([300] * 3, 0, [0] * 3)
  for fh, fl, word in ((hi_sum, lo_row, 1), (freq_hi, lo_row, 3),
                       (freq_hi, past, 6)):
    assert truth.bad_table(fh, fl, kmax) == word
    coder = Coder(device, fh, fl, kmax, rows)
    indices = dev(host, device)
    sizes, status = twice(lambda: coder.sizes(indices))
    assert (sizes == 0).all() and status.tolist() == [0, 0, word]
    packed, status = twice(lambda: coder.pack(indices, [300] * 3, offsets,
                                              900))
    assert (packed == 0).all() and status.tolist() == [0, 0, word]
    got, used, status = coder.decodes_as_restated(
        np.full(900, 7, np.uint8), offsets, b)
    assert status == [0, 0, word] and (got == -1).all() and (used == 0).all()
  # one symbol more in the table and the same row is fine
  coder = Coder(device, freq_hi, past, kmax + 1, rows)
  _, status = coder.sizes(dev(host, device))
  assert status.tolist() == [0, 0, 0]


# ------------------------------------------------------------ R-D entries
def _restated_rate(scal_indices, scal_freq, vec_indices, vec_tables, rows,
                   numel):
  scal_bytes = one_table.total_bytes(scal_indices.cpu().numpy(), scal_freq,
                                     rows if rows else 65536 //
                                     scal_indices.shape[1])
  top = len(vec_tables[0])
  streams, status = truth.encode(vec_indices.cpu().numpy(), *vec_tables,
                                 truth.LO * top, rows if rows else 65536)
  assert status == [0, 0, 0]
  return 8 * (scal_bytes + sum(len(s) for s in streams)) / float(numel)


def test_compute_RD_point_mixed_on_5000_codewords(device, scene):
  """A hand-made vector codebook of 5000 distinct rows, 256 of them the tails
  of the scene's rows and spread over all slots, so that codewords above 4096
  are in use."""
  from utils import vector_quantization as vq
  codes, patches, dictionary = (scene['codes'], scene['patches'],
                                scene['dictionary'])
  scal, vec = vq_data.SCAL_CLUSTS, vq_data.VEC_CLUST
  scal_at = torch.tensor(scal, device=device)
  vec_at = torch.tensor(vec, device=device)
  scal_codes = codes.index_select(1, scal_at).contiguous()
  vec_codes = codes.index_select(1, vec_at).contiguous()
  scal_cbook = vq._scalar._uniform_for(scal_codes, [WIDTH] * len(scal), MULT)

  rs = np.random.RandomState(23)
  k = 5000
  book = 400.0 * rs.randn(k, len(vec))
  book[0] = 0.0
  slots = 1 + (np.arange(256) * 2477) % (k - 1)       # 4999 is prime
  assert len(set(slots)) == 256 and slots.max() > 4096
  book[slots] = vec_codes.cpu().numpy().astype(np.float64)
  book[slots] += 1e-3 * rs.randn(256, len(vec))      # distinct rows
  assert len({row.tobytes() for row in book}) == k

  def point(**more):
    return vq.compute_RD_point_mixed(
        codes, patches, dictionary, scal, scal_cbook, vec, book,
        vec_max_codewords=LARGE, **more)
  split = {'source_code': 'ans_split', 'rows_per_stream': ROWS}
  rate, dist, tables = twice(lambda: point(**split))
  entropy_rate, entropy_dist = point(source_code='entropy')
  assert dist == entropy_dist

  scal_indices = vq.assign(scal_codes, scal_cbook)
  vec_indices = vq.vector_assign(vec_codes, book, max_codewords=LARGE)
  host = vec_indices.cpu().numpy()
  assert len(set(host[host > 4096].tolist())) > 10
  scal_freq, (freq_hi, freq_lo) = tables
  want_hi, want_lo = truth.frequencies(
      np.bincount(host, minlength=k).tolist(), k)
  assert np.array_equal(freq_hi, want_hi) and np.array_equal(freq_lo, want_lo)
  assert scal_freq.shape[0] == len(scal) and scal_freq.dtype == np.uint16
  want = _restated_rate(scal_indices, scal_freq, vec_indices,
                        (freq_hi, freq_lo), ROWS, scene['numel'])
  print('index_ans_split_rd ans_split %.6f entropy %.6f'
        % (rate, entropy_rate))
  assert rate == want and rate >= entropy_rate > 0
  # through the bytes: the same point
  assert twice(lambda: point(from_stream=True, **split)[:2]) == (rate, dist)
  # the default rows_per_stream, the tables given
  one = point(source_code='ans_split', tables=tables)
  assert one[2][0] is scal_freq and one[2][1][0] is freq_hi
  assert one[0] == _restated_rate(scal_indices, scal_freq, vec_indices,
                                  (freq_hi, freq_lo), None, scene['numel'])
  assert one[0] < rate and one[1] == dist
  # the table codes of 4096 symbols still refuse this codebook
  for source_code in ('ans', 'huffman'):
    with pytest.raises(NotImplementedError, match='trim_vector_codebook'):
      point(source_code=source_code)
  # the scalar-only entry does not know the name
  with pytest.raises(ValueError, match='source_code'):
    vq.compute_RD_point(codes, patches, dictionary,
                        vq._scalar._uniform_for(codes, [WIDTH] * 64, MULT),
                        source_code='ans_split')
  with pytest.raises(ValueError, match='from_stream'):
    point(source_code='entropy', from_stream=True)


def test_Mod3_training_and_test_call(device):
  """The scene of tests/vq_large_data.py from vec_init_num_bins = 100000: the
  codebook keeps its more than 4096 slots, the tables come back in the
  experiment's slots, and the test call with them gives the training point on
  the training data."""
  from utils import vector_quantization as vq
  s = vq_large_data.scene()
  codes, patches, dictionary = (dev(s[key], device) for key in
                                ('codes', 'patches', 'dictionary'))
  scal, vec = vq_data.SCAL_CLUSTS, vq_data.VEC_CLUST
  common = dict(vec_quant_multiplier=vq_large_data.RD_VEC_MULT,
                vec_max_codewords=LARGE, source_code='ans_split')

  def train(**more):
    return vq.Mod3_compute_RD_point(
        codes, patches, dictionary, scal, vec,
        scal_quant_multiplier=vq_large_data.RD_SCAL_MULT,
        scal_binwidths=[vq_data.SCAL_WIDTH] * len(scal),
        vec_init_num_bins=100000,
        max_iterations=vq_large_data.RD_ITERATIONS,
        epsilon=vq_large_data.RD_EPSILON, **more)
  out = train(**common)
  rate, dist, scal_cbook, vec_cbook, vec_cw_len, tab1, tab2, tab3 = out
  slots = vec_cbook['codebook'].shape[0]
  assert slots > 4096 and vec_cw_len is vec_cbook['lengths']   # not trimmed
  assert tab3 is None and tab1.dtype == np.uint16
  assert tab1.shape[0] == len(scal)
  freq_hi, freq_lo = tab2
  assert freq_hi.shape == (truth.hi_symbols(slots),)
  assert freq_lo.shape == (truth.hi_symbols(slots), truth.LO)
  plain = train(vec_quant_multiplier=vq_large_data.RD_VEC_MULT,
                vec_max_codewords=LARGE)
  assert plain[1] == dist and rate >= plain[0] > 0
  for key in ('codebook', 'k', 'lengths'):
    assert torch.equal(plain[3][key], vec_cbook[key]), key

  vec_indices = vq.vector_assign(
      codes.index_select(1, torch.tensor(vec, device=device)).contiguous(),
      vec_cbook, vec_cw_len, vq_large_data.RD_VEC_MULT, max_codewords=LARGE)
  host = vec_indices.cpu().numpy()
  k = int(vec_cbook['k'])
  want_hi, want_lo = truth.frequencies(
      np.bincount(host, minlength=slots).tolist(), k)
  assert np.array_equal(freq_hi, want_hi) and np.array_equal(freq_lo, want_lo)
  streams, status = truth.encode(host, freq_hi, freq_lo,
                                 truth.LO * len(freq_hi), 65536)
  assert status == [0, 0, 0]
  vec_bytes = sum(len(data) for data in streams)
  scal_indices = vq.assign(
      codes.index_select(1, torch.tensor(scal, device=device)).contiguous(),
      scal_cbook, scal_cbook['lengths'], scal_cbook['lagrange_mult'])
  from utils import index_coding
  scal_bytes = int(index_coding.index_ans_stream_bytes(scal_indices,
                                                       tab1).sum())
  assert rate == 8 * (scal_bytes + vec_bytes) / float(patches.numel())

  def test_call(**more):
    return vq.Mod3_compute_RD_point(
        codes, patches, dictionary, scal, vec,
        precomputed_scal_codebook=scal_cbook,
        precomputed_vec_codebook=vec_cbook,
        precomputed_vec_codebook_lengths=vec_cw_len, **common, **more)
  tabs = {'precomputed_huff_tab1': tab1, 'precomputed_huff_tab2': tab2}
  assert twice(lambda: test_call(**tabs)) == (rate, dist)
  assert test_call(from_stream=True, **tabs) == (rate, dist)
  for tables in ({}, {'precomputed_huff_tab1': tab1},
                 {'precomputed_huff_tab2': tab2}):
    with pytest.raises(ValueError, match='frequencies'):
      test_call(**tables)
  # 'ans' on the same codebook still raises
  with pytest.raises(NotImplementedError, match='trim_vector_codebook'):
    vq.Mod3_compute_RD_point(
        codes, patches, dictionary, scal, vec,
        vec_quant_multiplier=vq_large_data.RD_VEC_MULT,
        precomputed_scal_codebook=scal_cbook,
        precomputed_vec_codebook=vec_cbook,
        precomputed_vec_codebook_lengths=vec_cw_len,
        precomputed_huff_tab1=tab1, precomputed_huff_tab2=freq_hi,
        source_code='ans', vec_max_codewords=LARGE)
  # Mod2 takes the name the same way
  mod2 = vq.Mod2_compute_RD_point(
      codes, patches, dictionary, scal, vec,
      scal_quant_multiplier=vq_large_data.RD_SCAL_MULT,
      scal_binwidths=[vq_data.SCAL_WIDTH] * len(scal),
      vec_init_num_bins=100000, max_iterations=vq_large_data.RD_ITERATIONS,
      epsilon=vq_large_data.RD_EPSILON, from_stream=True, **common)
  assert mod2[3]['codebook'].shape[0] == slots
  assert np.array_equal(mod2[6][0], freq_hi)
  assert np.array_equal(mod2[6][1], freq_lo)
