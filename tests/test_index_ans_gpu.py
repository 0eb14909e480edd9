"""vtc_index_ans_sizes / _pack / _unpack (include/vtc_index_ans.h) and their
Python interface against the restatement of tests/index_ans_data.py, byte for
byte and index for index, every call twice; then source_code='ans' of the
rate-distortion entries and the two rate conditions of the sparse scene.  All
comparisons are between integers or bytes.

The raw calls run with outputs pre-filled with a pattern the call has to
overwrite and with a 0xFF-filled workspace of exactly the queried size."""
import ctypes

import numpy as np
import pytest
import torch

import index_ans_data as truth
import index_code_data as huffman
import vq_data

pytestmark = pytest.mark.gpu

OK = 0
LEADS = (0, 3)


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


def device_freq(freq, device):
  return dev(np.ascontiguousarray(freq).view(np.int16), device)


def _workspace(lib, m, kmax, device):
  need = lib.vtc_index_ans_workspace_bytes(m, kmax)
  assert need > 0
  return torch.full((need,), 0xFF, dtype=torch.uint8, device=device)


def raw_sizes(device, indices, freq, rows):
  """(stream_bytes, status) as numpy arrays."""
  import vtc_hip
  lib = vtc_hip.load_library()
  b, m = indices.shape
  kmax = freq.shape[1]
  n = truth.streams_of(b, rows)
  sizes = torch.full((n,), -7, dtype=torch.int32, device=device)
  status = torch.full((3,), -7, dtype=torch.int64, device=device)
  ws = _workspace(lib, m, kmax, device)
  rc = lib.vtc_index_ans_sizes(p(indices), b, m, p(freq), kmax, rows, p(sizes),
                               p(status), p(ws), ws.numel(),
                               vtc_hip.current_stream(device))
  assert rc == OK, lib.vtc_last_error()
  return sizes.cpu().numpy(), status.cpu().numpy()


def raw_pack(device, indices, freq, rows, sizes, offsets, nbytes, spare=64):
  """(packed [nbytes], status) as numpy arrays; `packed` pre-filled with ones
  and followed by `spare` bytes that must keep them."""
  import vtc_hip
  lib = vtc_hip.load_library()
  b, m = indices.shape
  kmax = freq.shape[1]
  packed = torch.full((nbytes + spare,), 0xFF, dtype=torch.uint8,
                      device=device)
  status = torch.full((3,), -7, dtype=torch.int64, device=device)
  ws = _workspace(lib, m, kmax, device)
  rc = lib.vtc_index_ans_pack(p(indices), b, m, p(freq), kmax, rows, p(sizes),
                              p(offsets), p(packed), nbytes, p(status), p(ws),
                              ws.numel(), vtc_hip.current_stream(device))
  assert rc == OK, lib.vtc_last_error()
  host = packed.cpu().numpy()
  assert (host[nbytes:] == 0xFF).all(), 'a store landed past packed_bytes'
  return host[:nbytes], status.cpu().numpy()


def raw_unpack(device, packed, offsets, b, m, freq, rows):
  """(indices, used_bytes, status) as numpy arrays."""
  import vtc_hip
  lib = vtc_hip.load_library()
  kmax = freq.shape[1]
  n = truth.streams_of(b, rows)
  indices = torch.full((b, m), -7, dtype=torch.int32, device=device)
  used = torch.full((n,), -7, dtype=torch.int32, device=device)
  status = torch.full((3,), -7, dtype=torch.int64, device=device)
  ws = _workspace(lib, m, kmax, device)
  rc = lib.vtc_index_ans_unpack(p(packed), packed.numel(), p(offsets), b, m,
                                p(freq), kmax, rows, p(indices), p(used),
                                p(status), p(ws), ws.numel(),
                                vtc_hip.current_stream(device))
  assert rc == OK, lib.vtc_last_error()
  return indices.cpu().numpy(), used.cpu().numpy(), status.cpu().numpy()


# ------------------------------------------------------------ exact streams
@pytest.mark.parametrize('case', truth.CASES, ids=truth.IDS)
def test_sizes_streams_and_the_way_back(device, case):
  from utils import index_coding
  b, m, kmax, rows = case
  host, host_freq = truth.case_indices(*case), truth.case_freq(*case)
  streams = truth.case_streams(*case)
  want_sizes = np.array([len(s) for s in streams], np.int32)
  n = len(streams)
  indices, freq = dev(host, device), device_freq(host_freq, device)

  sizes, status = twice(lambda: raw_sizes(device, indices, freq, rows))
  assert np.array_equal(sizes, want_sizes) and sizes.dtype == np.int32
  assert status.tolist() == [0, 0, 0]

  for lead in LEADS:
    offsets = truth.layout(want_sizes, lead, truth.gaps(n))
    nbytes = int(offsets[-1])
    want, skipped = truth.image(streams, offsets, nbytes)
    assert skipped == 0
    packed, status = twice(lambda: raw_pack(
        device, indices, freq, rows, dev(want_sizes, device),
        dev(offsets, device), nbytes))
    assert status.tolist() == [0, 0, 0]
    # every stream in its place, every byte outside the streams zero
    assert np.array_equal(packed, want), (case, lead)
    got, used, status = twice(lambda: raw_unpack(
        device, dev(want, device), dev(offsets, device), b, m, freq, rows))
    assert status.tolist() == [0, 0, 0]
    assert np.array_equal(got, host) and np.array_equal(used, want_sizes)

  # the Python interface: byte offsets from jpeg.bit_offsets, no gaps
  got_sizes = twice(lambda: index_coding.index_ans_stream_bytes(
      indices, host_freq, rows))
  assert got_sizes.dtype == torch.int32
  assert np.array_equal(got_sizes.cpu().numpy(), want_sizes)
  packed, offsets, got_rows = twice(lambda: index_coding.pack_index_ans(
      indices, host_freq, rows))
  assert got_rows == rows
  assert packed.dtype == torch.uint8 and offsets.dtype == torch.int64
  assert np.array_equal(offsets.cpu().numpy(),
                        truth.layout(want_sizes, 0, [0] * n))
  assert packed.cpu().numpy().tobytes() == b''.join(streams)
  back = twice(lambda: index_coding.unpack_index_ans(
      packed, offsets, host_freq, b, rows))
  assert back.dtype == torch.int32 and np.array_equal(back.cpu().numpy(), host)


def test_the_default_rows_per_stream(device):
  from utils import index_coding
  case = (257, 42, 64, 1)
  host, host_freq = truth.case_indices(*case), truth.case_freq(*case)
  indices = dev(host, device)
  packed, offsets, rows = index_coding.pack_index_ans(indices, host_freq)
  assert rows == 65536 // 42 and offsets.shape[0] == 2
  streams, _ = truth.encode(host, host_freq, rows)
  assert packed.cpu().numpy().tobytes() == b''.join(streams)
  back = index_coding.unpack_index_ans(packed, offsets, host_freq, 257, None)
  assert np.array_equal(back.cpu().numpy(), host)
  # bytes left over in a slot are reported, and refused only on request
  longer = torch.cat([packed, torch.zeros(6, dtype=torch.uint8,
                                          device=device)])
  wide = offsets + torch.tensor([0, 6], device=device)
  with pytest.raises(ValueError, match='do not use up'):
    index_coding.unpack_index_ans(longer, wide, host_freq, 257, rows)
  back = index_coding.unpack_index_ans(longer, wide, host_freq, 257, rows,
                                       exact=False)
  assert np.array_equal(back.cpu().numpy(), host)
  with pytest.raises(ValueError):
    index_coding.pack_index_ans(indices, host_freq, (1 << 24) // 42 + 1)
  with pytest.raises(ValueError, match='sum to'):
    wrong = host_freq.copy()
    wrong[5, 0] += 1
    index_coding.pack_index_ans(indices, wrong)


# ------------------------------------------------------------ bounded stores
def test_a_buffer_one_byte_short(device):
  """The last stream does not fit: it is skipped whole and counted, and
  nothing lands outside."""
  case = (257, 42, 1024, 100)
  b, m, kmax, rows = case
  streams = truth.case_streams(*case)
  sizes = np.array([len(s) for s in streams], np.int32)
  offsets = truth.layout(sizes, 3, truth.gaps(3)[:2] + [0])
  nbytes = int(offsets[-1]) - 1
  want, skipped = truth.image(streams, offsets, nbytes)
  assert skipped == 1 and (want[offsets[2]:] == 0).all()
  packed, status = twice(lambda: raw_pack(
      device, dev(truth.case_indices(*case), device),
      device_freq(truth.case_freq(*case), device), rows, dev(sizes, device),
      dev(offsets, device), nbytes))
  assert status.tolist() == [0, 0, 1]
  assert np.array_equal(packed, want)


def test_slots_and_sizes_that_are_not_the_coders(device):
  """A slot that overlaps the next, a negative offset, a size below the 256
  bytes of states and an odd one skip the stream before any store; a size two
  bytes short of the coder's own is counted, written inside its slot only,
  and leaves the neighbours intact."""
  case = (257, 42, 64, 40)     # 7 streams
  b, m, kmax, rows = case
  host, host_freq = truth.case_indices(*case), truth.case_freq(*case)
  streams, _ = truth.encode(host, host_freq, rows)
  n = len(streams)
  assert n == 7
  own = np.array([len(s) for s in streams], np.int32)
  offsets = truth.layout(own, 5, [0] * n)
  indices, freq = dev(host, device), device_freq(host_freq, device)
  nbytes = int(offsets[-1])

  sizes = own.copy()
  sizes[1] += 2          # passes offsets[2]
  sizes[2] = 254         # no room for the states
  sizes[3] -= 1          # odd
  sizes[5] -= 2          # one word short: counted, contents unspecified
  moved = offsets.copy()
  skipped = [1, 2, 3]
  packed, status = twice(lambda: raw_pack(
      device, indices, freq, rows, dev(sizes, device), dev(moved, device),
      nbytes))
  assert status.tolist() == [0, 0, 4]
  kept = [s if i not in skipped + [5] else b'\0' * len(s)
          for i, s in enumerate(streams)]
  want, _ = truth.image(kept, offsets, nbytes)
  outside_5 = np.ones(nbytes, bool)
  outside_5[offsets[5]:offsets[5] + sizes[5]] = False
  assert np.array_equal(packed[outside_5], want[outside_5])

  moved = offsets.copy()
  moved[0] = -1
  packed, status = raw_pack(device, indices, freq, rows, dev(own, device),
                            dev(moved, device), nbytes)
  assert status.tolist() == [0, 0, 1]
  want, _ = truth.image([b'\0' * len(streams[0])] + streams[1:], offsets,
                        nbytes)
  assert np.array_equal(packed, want)


# ---------------------------------------------------------- uncodable entries
def test_uncodable_entries(device):
  from utils import index_coding
  case = (257, 42, 64, 100)
  b, m, kmax, rows = case
  host_freq = truth.case_freq(*case)
  host = truth.case_indices(*case).copy()
  kinds = truth.column_kinds(b, m, kmax)
  gap = kinds.index('gap')
  assert host_freq[gap, 2] == 0 and host_freq[gap, 3] > 0
  host[3, 7] = -1              # the index of a NaN code
  host[3, 9] = kmax            # past the table
  host[150, gap] = 2           # a symbol of frequency 0
  host[256, 41] = -5
  streams, want_status = truth.encode(host, host_freq, rows)
  assert want_status == [4, 1 + 3 * m + 7, 0]
  want_sizes = np.array([len(s) for s in streams], np.int32)
  indices, freq = dev(host, device), device_freq(host_freq, device)
  sizes, status = twice(lambda: raw_sizes(device, indices, freq, rows))
  assert status.tolist() == want_status
  assert np.array_equal(sizes, want_sizes)
  offsets = truth.layout(want_sizes, 0, [0] * 3)
  packed, status = twice(lambda: raw_pack(
      device, indices, freq, rows, dev(want_sizes, device),
      dev(offsets, device), int(offsets[-1])))
  assert status.tolist() == want_status
  assert packed.tobytes() == b''.join(streams)
  with pytest.raises(KeyError, match='column 7 has no frequency for index -1'):
    index_coding.index_ans_stream_bytes(indices, host_freq, rows)
  with pytest.raises(KeyError, match=r'row 3'):
    index_coding.pack_index_ans(indices, host_freq, rows)
  # only the later ones: the first position moves
  host[3, 7], host[3, 9] = 0, 0
  _, want_status = truth.encode(host, host_freq, rows)
  assert want_status == [2, 1 + 150 * m + gap, 0]
  _, status = raw_sizes(device, dev(host, device), freq, rows)
  assert status.tolist() == want_status


# ------------------------------------------------------- decoder robustness
@pytest.fixture(scope='module')
def three_streams():
  case = (257, 42, 64, 100)
  host, freq = truth.case_indices(*case), truth.case_freq(*case)
  streams, _ = truth.encode(host, freq, case[3])
  sizes = [len(s) for s in streams]
  offsets = truth.layout(sizes, 0, [0, 0, 0])
  packed, _ = truth.image(streams, offsets, int(offsets[-1]))
  return case, host, freq, packed, offsets


def _decodes_as_restated(device, packed, offsets, b, m, host_freq, rows):
  want = truth.decode(packed, offsets, b, m, host_freq, rows)
  got, used, status = raw_unpack(device, dev(packed, device),
                                 dev(np.asarray(offsets, np.int64), device),
                                 b, m, device_freq(host_freq, device), rows)
  assert status.tolist() == want[2]
  assert np.array_equal(got, want[0]) and np.array_equal(used, want[1])
  return want


def test_a_slot_cut_by_two_bytes(device, three_streams):
  (b, m, kmax, rows), host, freq, packed, offsets = three_streams
  shifted = np.concatenate([packed[:offsets[2] - 2], packed[offsets[2]:]])
  moved = np.array([offsets[0], offsets[1], offsets[2] - 2, offsets[3] - 2])
  got, used, status = _decodes_as_restated(device, shifted, moved, b, m, freq,
                                           rows)
  assert status == [1, 2, 0]                   # the restatement, first
  assert np.array_equal(got[:100], host[:100])
  assert np.array_equal(got[200:], host[200:])
  assert (got[100:200] == -1).any() and used[1] <= moved[2] - moved[1]


def test_one_flipped_word(device, three_streams):
  (b, m, kmax, rows), host, freq, packed, offsets = three_streams
  flipped = packed.copy()
  flipped[offsets[1] + truth.HEADER + 10] ^= 0x40
  got, used, status = _decodes_as_restated(device, flipped, offsets, b, m,
                                           freq, rows)
  assert status[:2] == [1, 2]
  assert np.array_equal(got[:100], host[:100])
  assert np.array_equal(got[200:], host[200:])


def test_offsets_that_decrease(device, three_streams):
  (b, m, kmax, rows), host, freq, packed, offsets = three_streams
  wrong = offsets.copy()
  wrong[1] = offsets[2] + 4
  got, used, status = _decodes_as_restated(device, packed, wrong, b, m, freq,
                                           rows)
  assert status[0] >= 1 and (got[100:200] == -1).all() and used[1] == 0
  assert np.array_equal(got[200:], host[200:])
  # a negative one, and a buffer that ends inside the last stream's states
  wrong = offsets.copy()
  wrong[0] = -2
  _decodes_as_restated(device, packed, wrong, b, m, freq, rows)
  _decodes_as_restated(device, packed[:offsets[2] + 100], offsets, b, m, freq,
                       rows)


def test_a_bad_sum_column(device, three_streams):
  (b, m, kmax, rows), host, freq, packed, offsets = three_streams
  wrong = freq.copy()
  wrong[17, 0] += 1
  wrong[30, 1] += 1
  got, used, status = _decodes_as_restated(device, packed, offsets, b, m,
                                           wrong, rows)
  assert status == [0, 0, 18] and (got == -1).all() and (used == 0).all()
  indices, bad = dev(host, device), device_freq(wrong, device)
  sizes, status = raw_sizes(device, indices, bad, rows)
  assert status.tolist() == [0, 0, 18] and (sizes == 0).all()
  own = np.diff(offsets).astype(np.int32)
  image, status = raw_pack(device, indices, bad, rows, dev(own, device),
                           dev(offsets, device), len(packed))
  assert status.tolist() == [0, 0, 18] and (image == 0).all()


# ------------------------------------------------------------------- R-D
WIDTH, MULT = 5.0, 2.0
ROWS = 100         # 256 rows: streams of 100, 100 and 56


@pytest.fixture(scope='module')
def scene(device):
  """A 256 x 64 scene from the builder of tests/vq_data.py: its 32 patches
  eight times over, each copy under more seeded noise, against its dictionary,
  the codes made sparse by its thresholds; and a test set with another index
  distribution, as tests/test_index_code_gpu.py builds it (the rows in
  reverse, shrunk, the non-zero codes jittered)."""
  s = vq_data.scene()
  rs = np.random.RandomState(9)
  patches = np.concatenate([
      s['patches'] + 3.0 * copy * rs.randn(*s['patches'].shape)
      for copy in range(8)]).astype(np.float32)
  codes = patches.astype(np.float64) @ s['dictionary'].astype(np.float64).T
  threshold = np.full(64, 25.0)
  threshold[vq_data.VEC_CLUST] = 50.0
  codes[np.abs(codes) < threshold[None, :]] = 0.0
  assert patches.shape == codes.shape == (256, 64)
  assert np.array_equal(codes[:32].astype(np.float32), s['codes'])
  reverse = codes[::-1]
  test_codes = np.where(reverse != 0,
                        0.6 * reverse + rs.uniform(-30, 30, codes.shape), 0.0)
  on = {'codes': dev(codes.astype(np.float32), device),
        'patches': dev(patches, device),
        'dictionary': dev(s['dictionary'], device),
        'test_codes': dev(test_codes.astype(np.float32), device),
        'test_patches': dev(patches[::-1], device)}
  on['numel'] = patches.size
  return on


def restated_rate(indices, freq, rows, numel):
  host = indices.cpu().numpy()
  return 8 * truth.total_bytes(host, freq, rows) / float(numel)


def test_compute_RD_point_ans(device, scene):
  from utils import quantization
  codes, patches, dictionary = (scene['codes'], scene['patches'],
                                scene['dictionary'])
  codebook = quantization._uniform_for(codes, [WIDTH] * 64, MULT)
  kmax = codebook[0].shape[1]
  rate, dist, freq = twice(lambda: quantization.compute_RD_point(
      codes, patches, dictionary, codebook, source_code='ans',
      rows_per_stream=ROWS))
  entropy_rate, entropy_dist, none = quantization.compute_RD_point(
      codes, patches, dictionary, codebook, source_code='entropy')
  assert none is None and dist == entropy_dist

  indices = quantization.assign(codes, codebook)
  train = indices.cpu().numpy()
  counts = np.stack([np.bincount(train[:, j], minlength=kmax)
                     for j in range(64)])
  assert freq.dtype == np.uint16
  assert np.array_equal(freq, truth.frequency_array(
      counts, np.asarray(torch.as_tensor(codebook[1]).cpu())))
  assert rate == restated_rate(indices, freq, ROWS, scene['numel'])
  print('index_ans_rd train ans %.6f entropy %.6f' % (rate, entropy_rate))
  assert rate >= entropy_rate > 0
  # the default rows_per_stream: one stream of all 256 rows
  one = quantization.compute_RD_point(codes, patches, dictionary, codebook,
                                      source_code='ans', tables=freq)
  assert one[0] == restated_rate(indices, freq, 1024, scene['numel'])
  # two flushes less: 128 states of at least 16 bits each
  assert one[2] is freq and one[0] < rate

  # through the bytes: the same point
  assert twice(lambda: quantization.compute_RD_point(
      codes, patches, dictionary, codebook, source_code='ans',
      rows_per_stream=ROWS, from_stream=True)[:2]) == (rate, dist)

  # the test set under the trained frequencies: out-of-sample bytes
  test_indices = quantization.assign(scene['test_codes'], codebook)
  test = test_indices.cpu().numpy()
  unseen = [(r, j) for r in range(test.shape[0]) for j in range(64)
            if counts[j, test[r, j]] == 0]
  assert unseen, 'no test index is new: the weight-1 rule is not exercised'
  want = restated_rate(test_indices, freq, ROWS, scene['numel'])
  own = quantization.compute_RD_point(
      scene['test_codes'], scene['test_patches'], dictionary, codebook,
      source_code='ans', rows_per_stream=ROWS)
  test_rate, test_dist, same = twice(lambda: quantization.compute_RD_point(
      scene['test_codes'], scene['test_patches'], dictionary, codebook,
      source_code='ans', tables=freq, rows_per_stream=ROWS))
  assert same is freq and test_rate == want
  assert want > restated_rate(
      test_indices, truth.frequency_array(np.stack(
          [np.bincount(test[:, j], minlength=kmax) for j in range(64)]),
          np.asarray(torch.as_tensor(codebook[1]).cpu())), ROWS,
      scene['numel'])                              # on the CPU first
  print('index_ans_rd test trained %.6f own %.6f, %d unseen entries'
        % (test_rate, own[0], len(unseen)))
  assert test_rate > own[0] and test_dist == own[1]
  assert (test_rate, test_dist) == quantization.compute_RD_point(
      scene['test_codes'], scene['test_patches'], dictionary, codebook,
      source_code='ans', tables=freq, rows_per_stream=ROWS,
      from_stream=True)[:2]

  with pytest.raises(ValueError):
    quantization.compute_RD_point(codes, patches, dictionary, codebook,
                                  source_code='arithmetic')
  for source_code in ('entropy', 'jpeg'):
    with pytest.raises(ValueError, match='from_stream'):
      quantization.compute_RD_point(codes, patches, dictionary, codebook,
                                    source_code=source_code, from_stream=True)
  nan_codes = codes.clone()
  nan_codes[3, 5] = float('nan')
  with pytest.raises(ValueError):
    quantization.compute_RD_point(nan_codes, patches, dictionary, codebook,
                                  source_code='ans', tables=freq)


def test_baseline_and_Mod1_slots(device, scene):
  """huff_tab1 is the frequency array, huff_tab2 None; the test call
  reproduces compute_RD_point with those frequencies; from_stream gives the
  same point; codebooks without frequencies raise ValueError."""
  from utils import vector_quantization as quantization
  codes, patches, dictionary = (scene['codes'], scene['patches'],
                                scene['dictionary'])
  test_codes, test_patches = scene['test_codes'], scene['test_patches']
  ans = {'source_code': 'ans', 'rows_per_stream': ROWS}

  def train(**more):
    return quantization.baseline_compute_RD_point(
        codes, patches, dictionary, quant_multiplier=MULT,
        binwidths=[WIDTH] * 64, **ans, **more)
  rate, dist, codebook, tab1, tab2 = train()
  assert tab2 is None and tab1.dtype == np.uint16 and tab1.shape[0] == 64
  assert (rate, dist) == quantization.compute_RD_point(
      codes, patches, dictionary, codebook, **ans)[:2]
  assert rate == restated_rate(quantization.assign(codes, codebook), tab1,
                               ROWS, scene['numel'])
  assert train(from_stream=True)[:2] == (rate, dist)

  def test_call(**more):
    return quantization.baseline_compute_RD_point(
        test_codes, test_patches, dictionary, precomputed_codebook=codebook,
        precomputed_huff_tab1=tab1, precomputed_huff_tab2=tab2, **ans, **more)
  got = twice(test_call)
  assert got == quantization.compute_RD_point(
      test_codes, test_patches, dictionary, codebook, tables=tab1, **ans)[:2]
  assert got[0] == restated_rate(quantization.assign(test_codes, codebook),
                                 tab1, ROWS, scene['numel'])
  assert test_call(from_stream=True) == got
  with pytest.raises(ValueError, match='frequencies'):
    quantization.baseline_compute_RD_point(
        test_codes, test_patches, dictionary, precomputed_codebook=codebook,
        **ans)
  with pytest.raises(ValueError):
    quantization.baseline_compute_RD_point(
        codes, patches, dictionary, quant_multiplier=MULT,
        binwidths=[WIDTH] * 64, source_code='arithmetic')

  def mod1(**more):
    return quantization.Mod1_compute_RD_point(
        codes, patches, dictionary, quant_multiplier=MULT,
        init_binwidths=[WIDTH] * 64, max_iterations=vq_data.RD_ITERATIONS,
        epsilon=vq_data.RD_EPSILON, **ans, **more)
  rate, dist, codebook, lengths, tab1 = mod1()
  assert tab1.dtype == np.uint16 and tab1.shape[0] == 64
  k = codebook['k'].cpu().numpy()
  assert [int((row > 0).sum()) for row in tab1] == k.tolist()
  train_indices = quantization.assign(codes, codebook, lengths, MULT)
  assert rate == restated_rate(train_indices, tab1, ROWS, scene['numel'])
  assert mod1(from_stream=True)[:2] == (rate, dist)

  def mod1_test(**more):
    return quantization.Mod1_compute_RD_point(
        test_codes, test_patches, dictionary, quant_multiplier=MULT,
        precomputed_codebook=codebook, precomputed_codebook_lengths=lengths,
        **ans, **more)
  got = mod1_test(precomputed_huff_tab1=tab1)
  assert got[0] == restated_rate(
      quantization.assign(test_codes, codebook, lengths, MULT), tab1, ROWS,
      scene['numel'])
  assert mod1_test(precomputed_huff_tab1=tab1, from_stream=True) == got
  with pytest.raises(ValueError, match='frequencies'):
    mod1_test()


@pytest.mark.parametrize('variant', [2, 3])
def test_Mod2_and_Mod3_slots(device, scene, variant):
  """huff_tab1 = the scalar frequencies, huff_tab2 = the vector frequencies,
  huff_tab3 None; the rate is that of the combined (b, 41 + 1) index array,
  scalars first, under the frequencies padded to the larger kmax; the test
  call reproduces compute_RD_point_mixed; from_stream gives the same points."""
  from utils import vector_quantization as quantization
  codes, patches, dictionary = (scene['codes'], scene['patches'],
                                scene['dictionary'])
  test_codes, test_patches = scene['test_codes'], scene['test_patches']
  scal, vec = vq_data.SCAL_CLUSTS, vq_data.VEC_CLUST
  entry = (quantization.Mod2_compute_RD_point if variant == 2
           else quantization.Mod3_compute_RD_point)
  vec_mult = 3000.0
  ans = {'source_code': 'ans', 'rows_per_stream': ROWS}

  def train(**more):
    return entry(codes, patches, dictionary, scal, vec,
                 scal_quant_multiplier=MULT, scal_binwidths=[WIDTH] * len(scal),
                 vec_quant_multiplier=vec_mult, vec_init_num_bins=100000,
                 max_iterations=vq_data.RD_ITERATIONS,
                 epsilon=vq_data.RD_EPSILON, **more)
  out = train(**ans)
  rate, dist, scal_cbook, vec_cbook, vec_cw_len, tab1, tab2, tab3 = out
  assert tab3 is None and tab1.dtype == tab2.dtype == np.uint16
  assert tab1.shape[0] == len(scal) and tab2.ndim == 1
  assert int((tab2 > 0).sum()) == int(vec_cbook['k'])
  assert train(from_stream=True, **ans)[:2] == (rate, dist)
  plain = train(source_code='entropy')
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

  kmax = max(tab1.shape[1], tab2.shape[0])
  stacked = np.zeros((len(scal) + 1, kmax), np.uint16)
  stacked[:-1, :tab1.shape[1]] = tab1
  stacked[-1, :tab2.shape[0]] = tab2
  assert rate == restated_rate(combined(codes), stacked, ROWS, scene['numel'])

  def test_call(**more):
    return entry(test_codes, test_patches, dictionary, scal, vec,
                 vec_quant_multiplier=vec_mult,
                 precomputed_scal_codebook=scal_cbook,
                 precomputed_vec_codebook=vec_cbook,
                 precomputed_vec_codebook_lengths=vec_cw_len, **ans, **more)
  tabs = {'precomputed_huff_tab1': tab1, 'precomputed_huff_tab2': tab2}
  got = twice(lambda: test_call(precomputed_huff_tab3=tab3, **tabs))
  want = quantization.compute_RD_point_mixed(
      test_codes, test_patches, dictionary, scal, scal_cbook, vec, vec_cbook,
      tables=(tab1, tab2), **ans, **mixed)
  assert len(want) == 3 and got == want[:2]
  assert want[2][0] is tab1 and want[2][1] is tab2
  assert got[0] == restated_rate(combined(test_codes), stacked, ROWS,
                                 scene['numel'])
  assert test_call(from_stream=True, **tabs) == got
  assert quantization.compute_RD_point_mixed(
      test_codes, test_patches, dictionary, scal, scal_cbook, vec, vec_cbook,
      tables=(tab1, tab2), from_stream=True, **ans, **mixed)[:2] == got
  for tables in ({}, {'precomputed_huff_tab1': tab1},
                 {'precomputed_huff_tab2': tab2}):
    with pytest.raises(ValueError, match='frequencies'):
      test_call(**tables)


# ------------------------------------------------------------------- rates
def test_rate_conditions_on_the_sparse_scene(device):
  """About 90 % zeros: the device's range-coded bytes are strictly below the
  Huffman bits of the same indices under index_huffman_tables, and not below
  the in-sample entropy.  tests/test_index_ans_host.py asserts both for the
  restatement first; here the device bytes ARE the restatement's."""
  from utils import index_coding
  b, m, kmax, rows = truth.RATE_SCENE
  host = truth.sparse_indices(11, b, m, kmax)
  indices = dev(host, device)
  counts = np.stack([np.bincount(host[:, j], minlength=kmax)
                     for j in range(m)])
  freq = index_coding.index_ans_frequencies(counts)
  assert np.array_equal(freq, truth.frequency_array(counts))
  tables = index_coding.index_huffman_tables(counts)
  assert int(huffman.row_bits(host, tables).sum()) > (
      8 * truth.total_bytes(host, freq, rows))        # on the CPU first
  packed, offsets, _ = index_coding.pack_index_ans(indices, freq, rows)
  streams, _ = truth.encode(host, freq, rows)
  assert packed.cpu().numpy().tobytes() == b''.join(streams)
  ans_bits = 8 * packed.numel()
  _, column_bits = index_coding.index_code_bits(indices, tables)
  huffman_bits = int(column_bits.sum())
  entropy = truth.entropy_bits(host, kmax)
  ideal = truth.ideal_bits(host, freq)
  print('index_ans_rate per index: entropy %.4f ideal %.4f ans %.4f '
        'huffman %.4f' % tuple(v / float(b * m) for v in
                               (entropy, ideal, ans_bits, huffman_bits)))
  assert ans_bits < huffman_bits
  assert ans_bits >= entropy
