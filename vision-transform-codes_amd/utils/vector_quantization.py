"""
`utils.quantization` with the vector quantiser of the experiment's "Mod2" and
"Mod3" variants (experiments/rate_distortion_sparse_coding.py:600-840): a few
dozen coefficients of a sparse code go through scalar quantisers, the sparse
tail (23 of 64 coefficients there) is quantised as one vector by an
entropy-constrained vector quantiser fitted on the device.  The module is a
superset of utils.quantization, so the experiment needs one changed line:

  from utils import vector_quantization as quantization

The hot paths are the kernels of csrc/vq.hip behind include/vtc_vq.h
(DESIGN.md 4.16); device tensors in, device tensors out.

A vector quantiser of (b, d) vectors is described by
  codebook   float64 (kmax, d)  the codewords; the slots past k are never read
  k          int32   [1]        codewords in use
  lengths    float64 [kmax]     bits per codeword (only read when the Lagrange
                                multiplier is non-zero)
Every function that takes `codebook` accepts the dictionary vector_lloyd
returns, the pair (codebook, k), or a (k, d) array alone; numpy arrays are
uploaded, device tensors are used as they are.

Argument convention.  The reference's arrays are (s, b), one column per
sample; this package's are (b, s), one row per sample, as everywhere else in
utils.quantization.

Where torch does arithmetic here: the two stated exceptions of
utils.quantization, in their vector form -- vector_lloyd forms the initial
lengths -log2(count / n) from integer counts with torch.log2, once per fit,
and gathers its single host read through one float64 torch.cat.  Everything
else torch does is plumbing: column gathers, index_copy_, views.
"""
import ctypes

import numpy as np
import torch

import vtc_hip
from utils import quantization as _scalar
from utils.quantization import *   # noqa: F401,F403  (a superset of it)
from utils.quantization import (   # noqa: F401  the names the experiment uses
    assign, scalar_lloyd, index_counts, dequantize_assignments, entropy_bits,
    uniform_codebooks, cbook_inds_of_zero_pts, compute_RD_point,
    jpeg_compute_RD_point, baseline_compute_RD_point, Mod1_compute_RD_point)

VQ_MAX_DIM = vtc_hip.VQ_MAX_DIM
VQ_MAX_CODEWORDS = vtc_hip.VQ_MAX_CODEWORDS


# ------------------------------------------------------------------ host side
def _initial_codebook_host(vectors, num_bins):
  """initial_vector_codebook on a (b, d) numpy array: float64 (k, d)."""
  vectors = np.asarray(vectors, dtype=np.float32)
  b, d = vectors.shape
  m = max(1, min(int(num_bins), b, VQ_MAX_CODEWORDS))
  picked = vectors[(np.arange(m, dtype=np.int64) * b) // m]
  picked = picked[~np.isnan(picked).any(1)]
  rows = np.concatenate([np.zeros((1, d), np.float32), picked])
  rows = np.where(rows == 0, np.float32(0.0), rows)          # -0.0 is 0.0
  keys = np.ascontiguousarray(rows).view(np.uint32).reshape(len(rows), d)
  _, first = np.unique(keys, axis=0, return_index=True)
  return rows[np.sort(first)][:VQ_MAX_CODEWORDS].astype(np.float64)


def _vectors(vectors, name='vectors'):
  vectors = vtc_hip.require_device_tensor(vectors, name)
  if vectors.dim() != 2 or vectors.numel() == 0:
    raise ValueError('%s must be (b, d), got shape %s'
                     % (name, tuple(vectors.shape)))
  if vectors.shape[1] > VQ_MAX_DIM:
    raise NotImplementedError('d = %d, at most %d'
                              % (vectors.shape[1], VQ_MAX_DIM))
  return vectors.contiguous()


def _device_codebook(codebook, d, device):
  """(codebook float64 (kmax, d), k int32 [1], lengths or None) on `device`."""
  lengths, k = None, None
  if isinstance(codebook, dict):
    lengths = codebook.get('lengths')
    codebook, k = codebook['codebook'], codebook['k']
  elif isinstance(codebook, (tuple, list)) and len(codebook) == 2:
    codebook, k = codebook
  if len(codebook.shape) != 2 or codebook.shape[1] != d:
    raise ValueError('codebook must be (kmax, %d), got shape %s'
                     % (d, tuple(codebook.shape)))
  kmax = int(codebook.shape[0])
  if kmax < 1:
    raise ValueError('codebook must hold at least one codeword')
  if kmax > VQ_MAX_CODEWORDS:
    raise NotImplementedError('kmax = %d, at most %d'
                              % (kmax, VQ_MAX_CODEWORDS))
  if k is None:
    k = np.array([kmax], np.int32)
  elif not torch.is_tensor(k):
    k = np.asarray(k, dtype=np.int32).reshape(1)
  return (_scalar._on(device, codebook, torch.float64, (kmax, d), 'codebook'),
          _scalar._on(device, k, torch.int32, (1,), 'k'), lengths)


# ---------------------------------------------------------------- device side
def initial_vector_codebook(vectors, num_bins):
  """A deterministic starting codebook for vector_lloyd: float64 (k, d) device
  tensor whose row 0 is the zero vector.

  The candidates are the rows floor(i * b / m), i = 0 .. m - 1, of the (b, d)
  float32 device tensor `vectors`, with m = min(num_bins, b, 4096); rows with
  a NaN are skipped, the zero vector is put in front, bitwise duplicates are
  removed (first occurrences stay, -0.0 counts as 0.0) and at most 4096 rows
  are kept.  Plumbing: a gather on the device, the comparison of at most 4097
  rows on the host.

  The cap is a stated deviation: the experiment passes
  vec_init_num_bins = 100000, include/vtc_vq.h stops at 4096 codewords
  (DESIGN.md 7)."""
  vectors = _vectors(vectors)
  b = vectors.shape[0]
  m = max(1, min(int(num_bins), b, VQ_MAX_CODEWORDS))
  # the same rows as _initial_codebook_host picks: floor(i * b / m) of m rows
  rows = (torch.arange(m, dtype=torch.int64, device=vectors.device) * b) // m
  picked = vectors.index_select(0, rows).cpu().numpy()
  return torch.from_numpy(_initial_codebook_host(picked, m)).to(vectors.device)


def vector_assign(vectors, codebook, lengths=None, lagrange_mult=0.0,
                  return_dequantized=False):
  """indices [b] int32: for every row of the (b, d) float32 device tensor the
  lowest index i < k that minimises |x - c_i|^2 + lagrange_mult * lengths[i]
  in float64, the squared distance accumulated component by component
  (include/vtc_vq.h); with lagrange_mult == 0 the nearest codeword, lengths
  unused.  Ties go to the lowest index; a row with a NaN gets -1.  With
  return_dequantized also the (b, d) float32 codewords.  Only enqueues."""
  out = _vector_assign(vectors, codebook, lengths, lagrange_mult,
                       return_dequantized)
  return (out[0], out[1]) if return_dequantized else out[0]


def _vector_assign(vectors, codebook, lengths, lagrange_mult,
                   return_dequantized):
  lib = vtc_hip.load_library()
  vectors = _vectors(vectors)
  b, d = vectors.shape
  device = vectors.device
  values, k, own_lengths = _device_codebook(codebook, d, device)
  kmax = values.shape[0]
  if lengths is None:
    lengths = own_lengths
  if lagrange_mult != 0 and lengths is None:
    raise ValueError('a non-zero lagrange_mult needs the codeword lengths')
  if lagrange_mult == 0:
    lengths = None
  if lengths is not None:
    lengths = _scalar._on(device, lengths, torch.float64, (kmax,), 'lengths')
  indices = torch.empty(b, dtype=torch.int32, device=device)
  dequantized = (torch.empty((b, d), dtype=torch.float32, device=device)
                 if return_dequantized else None)
  status = torch.empty(1, dtype=torch.int64, device=device)
  vtc_hip.check(lib.vtc_vq_assign(
      vtc_hip.ptr(vectors), b, d, vtc_hip.ptr(values), vtc_hip.ptr(lengths),
      vtc_hip.ptr(k), kmax, float(lagrange_mult), vtc_hip.ptr(indices),
      vtc_hip.ptr(dequantized), vtc_hip.ptr(status),
      vtc_hip.current_stream(device)), 'vtc_vq_assign')
  return indices, dequantized, status


def vector_index_counts(indices, kmax):
  """int64 [kmax] device tensor: how often each index 0 .. kmax - 1 occurs in
  the [b] int32 device tensor `indices`; the -1 of a NaN row is not counted.
  Only enqueues."""
  lib = vtc_hip.load_library()
  indices = vtc_hip.require_device_tensor(indices, 'indices', torch.int32)
  if indices.dim() != 1 or indices.numel() == 0:
    raise ValueError('indices must be [b], got shape %s'
                     % (tuple(indices.shape),))
  indices = indices.contiguous()
  kmax = int(kmax)
  counts = torch.empty(max(kmax, 1), dtype=torch.int64, device=indices.device)
  vtc_hip.check(lib.vtc_vq_index_counts(
      vtc_hip.ptr(indices), indices.shape[0], kmax, vtc_hip.ptr(counts),
      vtc_hip.current_stream(indices.device)), 'vtc_vq_index_counts')
  return counts


def vector_dequantize(indices, codebook):
  """(b, d) float32 device tensor of codebook[indices[r]] rounded once to
  float32, a row of NaN where the index is -1.  A gather: tensor plumbing done
  by torch on the tensor's device.  Only enqueues."""
  indices = vtc_hip.require_device_tensor(indices, 'indices', torch.int32)
  if indices.dim() != 1:
    raise ValueError('indices must be [b], got shape %s'
                     % (tuple(indices.shape),))
  if isinstance(codebook, dict):
    codebook = codebook['codebook']
  elif isinstance(codebook, (tuple, list)) and len(codebook) == 2:
    codebook = codebook[0]
  values, _, _ = _device_codebook(codebook, codebook.shape[1], indices.device)
  picked = values.index_select(0, indices.clamp(min=0).to(torch.int64))
  picked = picked.to(torch.float32)
  return torch.where((indices < 0)[:, None],
                     torch.full_like(picked, float('nan')), picked)


def _state(tensors):
  return vtc_hip.VqState(**{name: t.data_ptr()
                            for name, t in tensors.items()})


def vector_lloyd(vectors, init_codebook, lagrange_mult=0.0, max_iterations=50,
                 epsilon=1e-5, pin_zero=True):
  """An entropy-constrained vector quantiser for the rows of the (b, d)
  float32 device tensor `vectors`, fitted on the device: the twin of
  scalar_lloyd.

  The fit starts from init_codebook ((k, d), e.g. initial_vector_codebook)
  with the lengths -log2(count / n) of the nearest-codeword assignment, then
  takes up to max_iterations steps of vtc_vq_lloyd_step: assign under
  |x - c|^2 + lagrange_mult * length, move every codeword to the mean of its
  members, drop the codewords without members, set length = -log2(count / n).
  The fit stops when its cost J = D + lagrange_mult * R improves by no more
  than epsilon * J; that test is made on the device, and the max_iterations
  steps are enqueued without a host read between them.  With pin_zero the
  codeword that is exactly the zero vector stays there and is never dropped.

  Returns a dictionary: 'codebook' float64 (kmax, d), 'lengths' float64
  [kmax], 'counts' int64 [kmax], 'k' int32 [1], 'zero_index' int32 [1] as
  device tensors (slots past k: 0.0, 0.0, 0), and, read once at the end,
  'iterations' (int), 'converged' (bool) and 'cost' float64 [3] = {J, D, R}
  of the last step (numpy).  A NaN in the vectors raises ValueError.
  """
  lib = vtc_hip.load_library()
  vectors = _vectors(vectors)
  b, d = vectors.shape
  device = vectors.device
  if isinstance(init_codebook, dict):
    init_codebook = (init_codebook['codebook'], init_codebook['k'])
  values, k, _ = _device_codebook(init_codebook, d, device)
  values, k = values.clone(), k.clone()      # the fit is in place
  kmax = values.shape[0]
  # the zero codeword of the start: plumbing (comparisons) on the device
  in_use = torch.arange(kmax, device=device) < k.to(torch.int64)
  is_zero = (values == 0).all(1) & in_use
  zero = torch.where(is_zero.any(), is_zero.to(torch.int32).argmax(),
                     torch.tensor(-1, device=device)).to(torch.int32)
  indices, _, first_status = _vector_assign(vectors, (values, k), None, 0.0,
                                            False)
  counts = vector_index_counts(indices, kmax)
  del indices
  # the first step's input lengths, by torch (module docstring)
  lengths = -torch.log2(counts.to(torch.float64) /
                        counts.sum().to(torch.float64))
  tensors = {
      'codebook': values, 'lengths': lengths.contiguous(), 'counts': counts,
      'cost': torch.zeros(3, dtype=torch.float64, device=device),
      'k': k, 'zero_index': zero.reshape(1).contiguous(),
      'active': torch.ones(1, dtype=torch.int32, device=device),
      'iterations': torch.zeros(1, dtype=torch.int32, device=device)}
  state = _state(tensors)
  status = torch.zeros(1, dtype=torch.int64, device=device)
  ws = vtc_hip.workspace(lib.vtc_vq_lloyd_step_workspace_bytes(b, d, kmax),
                         device)
  stream = vtc_hip.current_stream(device)
  for _ in range(int(max_iterations)):
    vtc_hip.check(lib.vtc_vq_lloyd_step(
        vtc_hip.ptr(vectors), b, d, kmax, float(lagrange_mult),
        float(epsilon), 1 if pin_zero else 0, ctypes.byref(state),
        ctypes.byref(state), vtc_hip.ptr(status), vtc_hip.ptr(ws), ws.numel(),
        stream), 'vtc_vq_lloyd_step')
  # the one read: everything as float64 in one buffer (module docstring)
  tail = torch.cat([tensors['active'].to(torch.float64),
                    tensors['iterations'].to(torch.float64),
                    tensors['cost'],
                    (status + first_status).to(torch.float64)]).cpu().numpy()
  if tail[-1] != 0:
    raise ValueError('vector_lloyd: the vectors hold NaN')
  result = {name: tensors[name] for name in
            ('codebook', 'k', 'lengths', 'counts', 'zero_index')}
  result['iterations'] = int(tail[1])
  result['converged'] = bool(tail[0] == 0)
  result['cost'] = tail[2:5].copy()
  return result


# ------------------------------------------------------------- rate-distortion
def _cluster(cluster, s, name):
  cluster = [int(c) for c in cluster]
  if not cluster:
    raise ValueError('%s is empty' % name)
  if min(cluster) < 0 or max(cluster) >= s:
    raise ValueError('%s falls outside [0, %d)' % (name, s))
  return cluster


def compute_RD_point_mixed(codes, patches, dictionary, scal_clusts,
                           scal_codebooks, vec_clust, vec_codebook,
                           scal_lengths=None, scal_lagrange_mult=0.0,
                           vec_lengths=None, vec_lagrange_mult=0.0,
                           fullimg_reshape_params=None, source_code='entropy',
                           tables=None, from_stream=False,
                           rows_per_stream=None):
  """One rate-distortion point of codes quantised in two parts.

  codes : (b, s) float32 device tensor; patches : (b, n); dictionary : (s, n),
  patches ~ codes @ dictionary.  The columns scal_clusts (a list of column
  numbers) go through quantization.assign with one scalar quantiser each
  (scal_codebooks, scal_lengths, scal_lagrange_mult: row j of the codebooks
  belongs to column scal_clusts[j]); the columns vec_clust are quantised as
  one vector per row by vector_assign (vec_codebook, vec_lengths,
  vec_lagrange_mult).  A coefficient in neither cluster is set to zero and
  costs no bits.  Overlapping clusters, or clusters that fall outside [0, s),
  raise ValueError.

  Returns (rate, distortion): the rate is (the sum over the scalar columns of
  the empirical entropy of their indices + the entropy of the vector indices)
  / patches.numel() in bits per pixel (entropy_bits); reconstruction and
  distortion are those of compute_RD_point.

  source_code 'huffman': the scalar indices and the vector index form one
  (b, len(scal_clusts) + 1) index array, scalars first in scal_clusts order,
  the vector column last, and every column is coded under a Huffman table of
  its own (utils.index_coding; the tables are padded to the larger kmax).
  `tables` = (scalar_tables, vector_table): a list of len(scal_clusts) dicts
  and one dict, trained on these indices when None.  The rate is the total of
  index_code_bits / patches.numel(), and a third value is returned: the
  tables.

  source_code 'ans': the same index array under the range coder of
  quantization.compute_RD_point.  `tables` = (scalar frequencies uint16
  (len(scal_clusts), kmax), vector frequencies uint16 (kmax',)), trained on
  these indices when None and padded with zeros to the larger kmax for the
  device; the rate is 8 x the bytes of the streams of rows_per_stream rows /
  patches.numel(), and the third value is that pair.

  from_stream (source_code 'huffman' and 'ans' only, ValueError otherwise):
  that index array is packed with index_coding.pack_index_streams
  (pack_index_ans) and read back by decode_codes_mixed; reconstruction and
  distortion are those of the decoded codes and the rate is the streams' total
  bits / patches.numel()."""
  _scalar._check_source_code(source_code)
  _scalar._check_from_stream(from_stream, source_code)
  codes = _scalar._codes(codes)
  patches = _scalar._codes(patches, 'patches')
  if patches.shape[0] != codes.shape[0]:
    raise ValueError('one patch per row of codes')
  b, s = codes.shape
  device = codes.device
  scal = _cluster(scal_clusts, s, 'scal_clusts')
  vec = _cluster(vec_clust, s, 'vec_clust')
  if len(set(scal + vec)) != len(scal) + len(vec):
    raise ValueError('scal_clusts and vec_clust overlap')
  scal_at = torch.tensor(scal, dtype=torch.int64, device=device)
  vec_at = torch.tensor(vec, dtype=torch.int64, device=device)

  scal_pair = _scalar._device_pair(scal_codebooks, len(scal), device)
  if scal_lengths is None and isinstance(scal_codebooks, dict):
    scal_lengths = scal_codebooks.get('lengths')
  scal_indices, scal_deq, scal_status = _scalar._assign(
      codes.index_select(1, scal_at).contiguous(), scal_pair, scal_lengths,
      scal_lagrange_mult, True)
  vec_values, vec_k, own_lengths = _device_codebook(vec_codebook, len(vec),
                                                    device)
  if vec_lengths is None:
    vec_lengths = own_lengths
  vec_indices, vec_deq, vec_status = _vector_assign(
      codes.index_select(1, vec_at).contiguous(), (vec_values, vec_k),
      vec_lengths, vec_lagrange_mult, True)

  dequantized = torch.zeros((b, s), dtype=torch.float32, device=device)
  dequantized.index_copy_(1, scal_at, scal_deq)
  dequantized.index_copy_(1, vec_at, vec_deq)
  if not from_stream:
    reconstruction = _scalar._reconstruct(dequantized, dictionary)
  if int(scal_status) != 0 or int(vec_status) != 0:
    raise ValueError('compute_RD_point_mixed: the codes hold NaN')
  if source_code == 'huffman':
    from utils import index_coding
    if tables is None:
      tables = (
          index_coding.index_huffman_tables(
              index_counts(scal_indices, scal_pair[0].shape[1]), scal_pair[1]),
          index_coding.index_huffman_tables(
              vector_index_counts(vec_indices, vec_values.shape[0]),
              vec_k)[0])
    scalar_tables, vector_table = tables
    streams = torch.cat([scal_indices, vec_indices[:, None]], 1)
    all_tables = list(scalar_tables) + [vector_table]
    if from_stream:
      total_bits, _, (packed, offsets) = _scalar._huffman_streams(
          streams, all_tables, None)
      reconstruction = _scalar._reconstruct(
          decode_codes_mixed(packed, offsets, all_tables, scal, scal_pair, vec,
                             (vec_values, vec_k), s), dictionary)
    else:
      total_bits, _ = _scalar._huffman_bits(streams, all_tables, None)
  elif source_code == 'ans':
    from utils import index_coding
    if tables is None:
      tables = (
          index_coding.index_ans_frequencies(
              index_counts(scal_indices, scal_pair[0].shape[1]), scal_pair[1]),
          index_coding.index_ans_frequencies(
              vector_index_counts(vec_indices, vec_values.shape[0]),
              vec_k)[0])
    scalar_tables, vector_table = tables
    streams = torch.cat([scal_indices, vec_indices[:, None]], 1)
    all_tables = _stacked_frequencies(scalar_tables, vector_table)
    if from_stream:
      total_bits, _, (packed, offsets, rows) = _scalar._ans_streams(
          streams, all_tables, None, rows_per_stream)
      reconstruction = _scalar._reconstruct(
          decode_codes_mixed(packed, offsets, all_tables, scal, scal_pair, vec,
                             (vec_values, vec_k), s, ans_shape=(b, rows)),
          dictionary)
    else:
      total_bits, _ = _scalar._ans_bits(streams, all_tables, None,
                                        rows_per_stream)
  else:
    total_bits = (
        entropy_bits(index_counts(scal_indices, scal_pair[0].shape[1])) +
        entropy_bits(vector_index_counts(vec_indices,
                                         vec_values.shape[0])[None, :]))
  rate = total_bits / float(patches.numel())
  distortion = _scalar._distortion(patches, reconstruction,
                                   fullimg_reshape_params)
  if source_code == 'huffman':
    return rate, distortion, (list(scalar_tables), vector_table)
  if source_code == 'ans':
    return rate, distortion, (scalar_tables, vector_table)
  return rate, distortion


def _stacked_frequencies(scalar_freq, vector_freq):
  """The uint16 (len(scal_clusts) + 1, kmax) frequencies of the combined index
  array: the scalar rows, then the vector row, padded with zeros (absent
  symbols) to the larger kmax."""
  scalar_freq = np.asarray(scalar_freq)
  vector_freq = np.asarray(vector_freq).reshape(1, -1)
  if scalar_freq.ndim != 2:
    raise ValueError('the scalar frequencies must be (len(scal_clusts), kmax)')
  kmax = max(scalar_freq.shape[1], vector_freq.shape[1])
  out = np.zeros((scalar_freq.shape[0] + 1, kmax), dtype=np.uint16)
  out[:-1, :scalar_freq.shape[1]] = scalar_freq
  out[-1, :vector_freq.shape[1]] = vector_freq[0]
  return out


def decode_codes_mixed(packed, offsets, tables, scal_clusts, scal_codebooks,
                       vec_clust, vec_codebook, s, ans_shape=None):
  """The (b, s) float32 dequantised codes whose index streams are in (packed,
  offsets), the layout compute_RD_point_mixed codes: one row per patch, the
  scalar indices first in scal_clusts order, the vector index last.  `tables`
  is the list of len(scal_clusts) + 1 tables in that order.
  index_coding.unpack_index_streams, then quantization.dequantize_assignments
  into the columns scal_clusts and vector_dequantize into the columns
  vec_clust; a column in neither cluster is zero.  One host read (the
  decoder's status).

  ans_shape = (b, rows_per_stream): the streams are those of
  index_coding.pack_index_ans, `tables` the uint16 (len(scal_clusts) + 1,
  kmax) frequencies in that order, read by index_coding.unpack_index_ans."""
  s = int(s)
  scal = _cluster(scal_clusts, s, 'scal_clusts')
  vec = _cluster(vec_clust, s, 'vec_clust')
  if len(set(scal + vec)) != len(scal) + len(vec):
    raise ValueError('scal_clusts and vec_clust overlap')
  if ans_shape is None:
    tables = list(tables)
  if len(tables) != len(scal) + 1:
    raise ValueError('%d tables for %d scalar columns and the vector column'
                     % (len(tables), len(scal)))
  indices = _scalar._unpack_indices(packed, offsets, tables, ans_shape)
  device = indices.device
  scal_deq = _scalar.dequantize_assignments(
      indices[:, :len(scal)].contiguous(), scal_codebooks)
  vec_deq = vector_dequantize(indices[:, len(scal)].contiguous(), vec_codebook)
  if vec_deq.shape[1] != len(vec):
    raise ValueError('vec_codebook must be (kmax, %d)' % len(vec))
  codes = torch.zeros((indices.shape[0], s), dtype=torch.float32,
                      device=device)
  codes.index_copy_(1, torch.tensor(scal, dtype=torch.int64, device=device),
                    scal_deq)
  codes.index_copy_(1, torch.tensor(vec, dtype=torch.int64, device=device),
                    vec_deq)
  return codes


def _gathered(codes, cluster):
  codes = _scalar._codes(codes)
  cluster = _cluster(cluster, codes.shape[1], 'cluster')
  at = torch.tensor(cluster, dtype=torch.int64, device=codes.device)
  return codes.index_select(1, at).contiguous()


def _fit_vector_part(codes, vec_clust, vec_quant_multiplier, vec_init_num_bins,
                     max_iterations, epsilon):
  vectors = _gathered(codes, vec_clust)
  return vector_lloyd(vectors,
                      initial_vector_codebook(vectors, vec_init_num_bins),
                      lagrange_mult=vec_quant_multiplier,
                      max_iterations=max_iterations, epsilon=epsilon)


def _mixed_point(who, training, source_code, from_stream, rows_per_stream,
                 huff_tab1, huff_tab2, *args, **kwargs):
  """compute_RD_point_mixed for Mod2 / Mod3: (rate, distortion, huff_tab1,
  huff_tab2), the two tables None under 'entropy'."""
  _scalar._check_source_code(source_code)
  _scalar._check_from_stream(from_stream, source_code)
  if source_code not in _scalar._TABLE_CODES:
    return compute_RD_point_mixed(*args, **kwargs) + (None, None)
  tables = None
  if not training:
    _scalar._need_tables(who, huff_tab1, huff_tab2, source_code=source_code)
    tables = (huff_tab1, huff_tab2)
  rate, distortion, tables = compute_RD_point_mixed(
      *args, source_code=source_code, tables=tables, from_stream=from_stream,
      rows_per_stream=rows_per_stream, **kwargs)
  return rate, distortion, tables[0], tables[1]


def Mod2_compute_RD_point(codes, patches, dictionary, scal_clusts, vec_clust,
                          scal_quant_multiplier=1.0, scal_binwidths=None,
                          vec_quant_multiplier=1.0, vec_init_num_bins=4096,
                          precomputed_scal_codebook=None,
                          precomputed_vec_codebook=None,
                          precomputed_vec_codebook_lengths=None,
                          precomputed_huff_tab1=None,
                          precomputed_huff_tab2=None,
                          precomputed_huff_tab3=None,
                          fullimg_reshape_params=None, max_iterations=50,
                          epsilon=1e-5, source_code='entropy',
                          from_stream=False, rows_per_stream=None):
  """The experiment's Mod2_compute_RD_point, with (b, s) codes (module
  docstring): the columns scal_clusts get uniform scalar codebooks of bin
  width scal_binwidths * scal_quant_multiplier (as in
  baseline_compute_RD_point), the columns vec_clust one entropy-constrained
  vector quantiser, vector_lloyd from initial_vector_codebook(.,
  vec_init_num_bins) with lagrange_mult = vec_quant_multiplier; every index
  stream is coded at its empirical entropy (compute_RD_point_mixed).

  Training call (no precomputed_*): returns the experiment's 8-tuple (rate,
  distortion, scal_cbook, vec_cbook, vec_cw_len, None, None, None): the pair
  of uniform_codebooks, the dictionary of vector_lloyd and its 'lengths'; the
  three Huffman table slots are None for the reason
  baseline_compute_RD_point's docstring gives (and the precomputed_huff_tab*
  arguments are accepted and unused).  Test call (precomputed_scal_codebook,
  precomputed_vec_codebook, precomputed_vec_codebook_lengths): returns
  (rate, distortion).

  With source_code='huffman' every index stream is coded under a Huffman
  table of its own instead (compute_RD_point_mixed).  The experiment's missing
  module never said what its three table slots held; here the training call
  returns huff_tab1 = the list of len(scal_clusts) scalar tables, huff_tab2 =
  the vector table, huff_tab3 = None, and a test call takes the first two back
  as precomputed_huff_tab1 and precomputed_huff_tab2 and measures the bits of
  the test indices under them.  Precomputed codebooks without both tables
  raise ValueError.  from_stream is that of compute_RD_point_mixed, and so
  are source_code='ans' and rows_per_stream: huff_tab1 and huff_tab2 are then
  the scalar and the vector frequency arrays."""
  training = precomputed_scal_codebook is None
  if training:
    scal_cbook = _scalar._uniform_for(_gathered(codes, scal_clusts),
                                      scal_binwidths, scal_quant_multiplier)
    vec_cbook = _fit_vector_part(codes, vec_clust, vec_quant_multiplier,
                                 vec_init_num_bins, max_iterations, epsilon)
    vec_cw_len = vec_cbook['lengths']
  else:
    scal_cbook, vec_cbook, vec_cw_len = (precomputed_scal_codebook,
                                         precomputed_vec_codebook,
                                         precomputed_vec_codebook_lengths)
  rate, distortion, huff_tab1, huff_tab2 = _mixed_point(
      'Mod2_compute_RD_point', training, source_code, from_stream,
      rows_per_stream,
      precomputed_huff_tab1, precomputed_huff_tab2,
      codes, patches, dictionary, scal_clusts, scal_cbook, vec_clust,
      vec_cbook, vec_lengths=vec_cw_len,
      vec_lagrange_mult=vec_quant_multiplier,
      fullimg_reshape_params=fullimg_reshape_params)
  if training:
    return (rate, distortion, scal_cbook, vec_cbook, vec_cw_len, huff_tab1,
            huff_tab2, None)
  return rate, distortion


def Mod3_compute_RD_point(codes, patches, dictionary, scal_clusts, vec_clust,
                          scal_quant_multiplier=1.0, scal_binwidths=None,
                          vec_quant_multiplier=1.0, vec_init_num_bins=4096,
                          precomputed_scal_codebook=None,
                          precomputed_vec_codebook=None,
                          precomputed_vec_codebook_lengths=None,
                          precomputed_huff_tab1=None,
                          precomputed_huff_tab2=None,
                          precomputed_huff_tab3=None,
                          fullimg_reshape_params=None, max_iterations=50,
                          epsilon=1e-5, source_code='entropy',
                          from_stream=False, rows_per_stream=None):
  """The experiment's Mod3_compute_RD_point: Mod2_compute_RD_point with
  entropy-constrained scalar quantisers, scalar_lloyd from uniform codebooks
  of bin width scal_binwidths with lagrange_mult = scal_quant_multiplier (as
  in Mod1_compute_RD_point).  The experiment's test call does not pass the
  scalar multiplier again, so the returned scal_cbook is scalar_lloyd's
  dictionary with one more key, 'lagrange_mult', and a test call assigns with
  that value and the dictionary's 'lengths'.  Returns as Mod2_compute_RD_point
  does, source_code='huffman' and 'ans', their table slots, from_stream and
  rows_per_stream included."""
  training = precomputed_scal_codebook is None
  if training:
    scal_codes = _gathered(codes, scal_clusts)
    scal_cbook = scalar_lloyd(
        scal_codes, _scalar._uniform_for(scal_codes, scal_binwidths, 1.0),
        lagrange_mult=scal_quant_multiplier, max_iterations=max_iterations,
        epsilon=epsilon)
    scal_cbook['lagrange_mult'] = scal_quant_multiplier
    vec_cbook = _fit_vector_part(codes, vec_clust, vec_quant_multiplier,
                                 vec_init_num_bins, max_iterations, epsilon)
    vec_cw_len = vec_cbook['lengths']
  else:
    scal_cbook, vec_cbook, vec_cw_len = (precomputed_scal_codebook,
                                         precomputed_vec_codebook,
                                         precomputed_vec_codebook_lengths)
  rate, distortion, huff_tab1, huff_tab2 = _mixed_point(
      'Mod3_compute_RD_point', training, source_code, from_stream,
      rows_per_stream,
      precomputed_huff_tab1, precomputed_huff_tab2,
      codes, patches, dictionary, scal_clusts, scal_cbook, vec_clust,
      vec_cbook, scal_lengths=scal_cbook['lengths'],
      scal_lagrange_mult=scal_cbook['lagrange_mult'], vec_lengths=vec_cw_len,
      vec_lagrange_mult=vec_quant_multiplier,
      fullimg_reshape_params=fullimg_reshape_params)
  if training:
    return (rate, distortion, scal_cbook, vec_cbook, vec_cw_len, huff_tab1,
            huff_tab2, None)
  return rate, distortion
