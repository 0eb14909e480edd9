"""
The `utils.quantization` module that the reference's experiments import
(experiments/rate_distortion_sparse_coding.py:24,
experiments/rate_distortion_jpeg.py) and the reference never shipped: scalar
quantisers with one codebook per code coefficient, the entropy-constrained
Lloyd fit of the experiment's "Mod1" variant, and the rate-distortion point of
quantised sparse codes.  The hot paths are the kernels of csrc/quantization.hip
behind include/vtc_quant.h; device tensors in, device tensors
out.

A quantiser of (b, s) codes is described by
  codebooks  float64 (s, kmax)  the codewords of each column; the slots past
                                k[j] are never read (uniform_codebooks pads
                                with +inf, a Lloyd step with 0.0)
  k          int32   [s]        codewords in use
  lengths    float64 (s, kmax)  bits per codeword (only read when the Lagrange
                                multiplier is non-zero)
Every function that takes `codebooks` accepts the pair (codebooks, k), the
dictionary scalar_lloyd returns, or an (s, kmax) array padded with +inf alone,
whose k is then the number of finite leading entries of each row; numpy arrays are
uploaded, device tensors are used as they are.

Where torch does arithmetic here.  The package's rule is that torch is
plumbing and arithmetic is a HIP kernel (vtc_hip).  Two places of this module
are stated exceptions, both outside the contract of include/vtc_quant.h and
its bitwise-reproducible outputs: scalar_lloyd forms the (s, kmax) initial
lengths -log2(count / n) from the integer counts of index_counts with
torch.log2 and a division on the device, once per fit -- they are the input of
the first step, not an output of the library, and are tied to numpy's only
through the margin the tests keep around every assignment; and its single
host read gathers active, iterations, cost and the status word through one
float64 torch.cat (int32 and the counts of NaN codes up to 2^53 are exact in
float64), so that a fit costs one device-to-host copy.

The vector quantiser of the experiment's Mod2 / Mod3 variants lives in
utils.vector_quantization (include/vtc_vq.h), a superset of
this module: `from utils import vector_quantization as quantization`.

The rate of a point is the cost of the JPEG source code, the empirical entropy
of the indices (the default of the baseline and Mod entries) or, with
source_code='huffman' or 'ans', the bits of the indices under Huffman tables
or range-coder frequencies that may have been trained on other data
(DESIGN.md 4.17, 4.19).  The entry points take a source code with tables as
its description in utils.index_coding.SOURCE_CODES and follow one path: train
when no tables are given, then total the bits, or pack, unpack and dequantise.
"""
import ctypes

import numpy as np
import torch

import vtc_hip
from utils import index_coding as _coding

MAX_CODEWORDS = vtc_hip.QUANT_MAX_CODEWORDS


# ------------------------------------------------------------------ host side
def uniform_codebooks(lo, hi, binwidths):
  """Uniform codebooks that cover [lo[j], hi[j]] with bins of binwidths[j]
  (host, numpy; lo and hi are what utils.plotting.code_summary returns as
  'min' and 'max').

  For column j, in float64: m_lo = rint(lo / w), m_hi = rint(hi / w) with ties
  to even, and c_i = (m_lo + i) * w for i = 0 .. m_hi - m_lo, so that 0.0 is a
  codeword whenever m_lo <= 0 <= m_hi.  A column whose lo or hi is NaN (nothing
  kept) gets the single codeword 0.0.

  Returns (codebooks float64 (s, kmax) padded with +inf, k int32 [s]).  More
  than 1024 codewords in a column raises ValueError.
  """
  lo = np.asarray(lo, dtype=np.float64).reshape(-1)
  hi = np.asarray(hi, dtype=np.float64).reshape(-1)
  w = np.asarray(binwidths, dtype=np.float64).reshape(-1)
  if w.size == 1:
    w = np.broadcast_to(w, lo.shape)
  if not (lo.shape == hi.shape == w.shape):
    raise ValueError('lo, hi and binwidths must have one entry per column')
  if not (np.isfinite(w).all() and (w > 0).all()):
    raise ValueError('binwidths must be finite and positive')
  empty = np.isnan(lo) | np.isnan(hi)
  lo, hi = np.where(empty, 0.0, lo), np.where(empty, 0.0, hi)
  if not (np.isfinite(lo).all() and np.isfinite(hi).all() and
          (lo <= hi).all()):
    raise ValueError('lo and hi must be finite with lo <= hi')
  m_lo, m_hi = np.rint(lo / w), np.rint(hi / w)
  count = m_hi - m_lo + 1
  for j in np.nonzero(count > MAX_CODEWORDS)[0]:
    raise ValueError('column %d needs %d codewords, at most %d'
                     % (j, int(count[j]), MAX_CODEWORDS))
  k = count.astype(np.int32)
  codebooks = np.full((len(k), int(k.max())), np.inf)
  for j in range(len(k)):
    codebooks[j, :k[j]] = (m_lo[j] + np.arange(k[j], dtype=np.float64)) * w[j]
  return codebooks, k


def _host_pair(codebooks):
  """(values float64 (s, kmax), k int32 [s]) on the host."""
  if isinstance(codebooks, dict):
    codebooks = (codebooks['codebooks'], codebooks['k'])
  k = None
  if isinstance(codebooks, (tuple, list)) and len(codebooks) == 2:
    codebooks, k = codebooks
  to_host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
  values = to_host(codebooks).astype(np.float64, copy=False)
  if values.ndim != 2:
    raise ValueError('codebooks must be (s, kmax), got shape %s'
                     % (values.shape,))
  if k is None:
    finite = np.isfinite(values)
    k = np.where(finite.all(1), values.shape[1], finite.argmin(1))
  return values, to_host(k).astype(np.int32).reshape(-1)


def cbook_inds_of_zero_pts(codebooks):
  """int32 [s]: for each column, the index of the codeword in use whose value
  is exactly 0.0 (the lowest, should there be several), or -1."""
  values, k = _host_pair(codebooks)
  is_zero = (values == 0.0) & (np.arange(values.shape[1])[None, :] < k[:, None])
  return np.where(is_zero.any(1), is_zero.argmax(1), -1).astype(np.int32)


# ---------------------------------------------------------------- device side
def _codes(codes, name='codes'):
  codes = vtc_hip.require_device_tensor(codes, name)
  if codes.dim() != 2 or codes.numel() == 0:
    raise ValueError('%s must be (b, s), got shape %s'
                     % (name, tuple(codes.shape)))
  return codes.contiguous()


def _on(device, array, dtype, shape, name):
  if torch.is_tensor(array):
    t = array.to(device=device, dtype=dtype)
  else:
    t = torch.from_numpy(np.ascontiguousarray(array)).to(device=device,
                                                         dtype=dtype)
  if tuple(t.shape) != tuple(shape):
    raise ValueError('%s must have shape %s, got %s'
                     % (name, tuple(shape), tuple(t.shape)))
  return t.contiguous()


def _device_pair(codebooks, s, device):
  """(values float64 (s, kmax), k int32 [s]) on `device`, kmax checked."""
  if isinstance(codebooks, dict):
    codebooks = (codebooks['codebooks'], codebooks['k'])
  if not (isinstance(codebooks, (tuple, list)) and len(codebooks) == 2):
    codebooks = _host_pair(codebooks)
  values, k = codebooks
  if len(values.shape) != 2 or values.shape[0] != s:
    raise ValueError('codebooks must be (%d, kmax), got shape %s'
                     % (s, tuple(values.shape)))
  kmax = int(values.shape[1])
  if kmax < 1:
    raise ValueError('codebooks must hold at least one codeword')
  if kmax > MAX_CODEWORDS:
    raise NotImplementedError('kmax = %d, at most %d' % (kmax, MAX_CODEWORDS))
  return (_on(device, values, torch.float64, (s, kmax), 'codebooks'),
          _on(device, k, torch.int32, (s,), 'k'))


def assign(codes, codebooks, lengths=None, lagrange_mult=0.0,
           return_dequantized=False):
  """indices (b, s) int32: for every code the lowest index i < k[j] that
  minimises (x - c[j, i])^2 + lagrange_mult * lengths[j, i] in float64
  (include/vtc_quant.h); with lagrange_mult == 0 the nearest codeword, lengths
  unused.  Ties go to the lowest index; a NaN code gets -1.  With
  return_dequantized also the (b, s) float32 codewords.  Only enqueues.
  """
  out = _assign(codes, codebooks, lengths, lagrange_mult, return_dequantized)
  return (out[0], out[1]) if return_dequantized else out[0]


def _assign(codes, codebooks, lengths, lagrange_mult, return_dequantized):
  lib = vtc_hip.load_library()
  codes = _codes(codes)
  b, s = codes.shape
  device = codes.device
  values, k = _device_pair(codebooks, s, device)
  kmax = values.shape[1]
  if lengths is None and isinstance(codebooks, dict):
    lengths = codebooks.get('lengths')
  if lagrange_mult != 0 and lengths is None:
    raise ValueError('a non-zero lagrange_mult needs the codeword lengths')
  if lagrange_mult == 0:
    lengths = None
  if lengths is not None:
    lengths = _on(device, lengths, torch.float64, (s, kmax), 'lengths')
  indices = torch.empty((b, s), dtype=torch.int32, device=device)
  dequantized = (torch.empty((b, s), dtype=torch.float32, device=device)
                 if return_dequantized else None)
  status = torch.empty(1, dtype=torch.int64, device=device)
  vtc_hip.check(lib.vtc_quant_assign(
      vtc_hip.ptr(codes), b, s, vtc_hip.ptr(values), vtc_hip.ptr(lengths),
      vtc_hip.ptr(k), kmax, float(lagrange_mult), vtc_hip.ptr(indices),
      vtc_hip.ptr(dequantized), vtc_hip.ptr(status),
      vtc_hip.current_stream(device)), 'vtc_quant_assign')
  return indices, dequantized, status


def index_counts(indices, kmax):
  """int64 (s, kmax) device tensor: how often each index 0 .. kmax - 1 occurs
  in each column of the (b, s) int32 device tensor `indices`; indices outside
  that range (the -1 of a NaN code) are not counted.  Only enqueues."""
  lib = vtc_hip.load_library()
  indices = vtc_hip.require_device_tensor(indices, 'indices', torch.int32)
  if indices.dim() != 2 or indices.numel() == 0:
    raise ValueError('indices must be (b, s), got shape %s'
                     % (tuple(indices.shape),))
  indices = indices.contiguous()
  b, s = indices.shape
  kmax = int(kmax)
  counts = torch.empty((s, max(kmax, 1)), dtype=torch.int64,
                       device=indices.device)
  vtc_hip.check(lib.vtc_quant_index_counts(
      vtc_hip.ptr(indices), b, s, kmax, vtc_hip.ptr(counts),
      vtc_hip.current_stream(indices.device)), 'vtc_quant_index_counts')
  return counts


def dequantize_assignments(indices, codebooks):
  """(b, s) float32 device tensor of codebooks[j, indices[r, j]] rounded once
  to float32, NaN where the index is -1.  A gather: tensor plumbing done by
  torch on the tensor's device.  Only enqueues."""
  indices = vtc_hip.require_device_tensor(indices, 'indices', torch.int32)
  if indices.dim() != 2:
    raise ValueError('indices must be (b, s), got shape %s'
                     % (tuple(indices.shape),))
  values, _ = _device_pair(codebooks, indices.shape[1], indices.device)
  picked = torch.gather(values.t(), 0, indices.clamp(min=0).to(torch.int64))
  picked = picked.to(torch.float32)
  return torch.where(indices < 0, torch.full_like(picked, float('nan')),
                     picked)


def _state(tensors):
  return vtc_hip.QuantState(**{name: t.data_ptr()
                               for name, t in tensors.items()})


def scalar_lloyd(codes, init_codebooks, lagrange_mult=0.0, max_iterations=50,
                 epsilon=1e-5, pin_zero=True):
  """Entropy-constrained scalar Lloyd quantisers, one per column of the
  (b, s) float32 device tensor `codes`, fitted on the device.

  The fit starts from init_codebooks with the lengths -log2(count / b) of the
  nearest-codeword assignment, then takes up to max_iterations steps of
  vtc_quant_lloyd_step: assign under (x - c)^2 + lagrange_mult * length,
  move every codeword to the mean of its members, drop the codewords without
  members, set length = -log2(count / n).  A column stops when its cost
  J = D + lagrange_mult * R improves by no more than epsilon * J; that test is
  made on the device, and the max_iterations steps are enqueued without a
  host read between them.  With pin_zero the codeword that is exactly 0.0
  stays 0.0 and is never dropped.

  Returns a dictionary: 'codebooks' float64 (s, kmax), 'lengths' float64
  (s, kmax), 'counts' int64 (s, kmax), 'k' int32 [s], 'zero_index' int32 [s]
  as device tensors (slots past k: 0.0, 0.0, 0), and, read once at the end,
  'iterations' int32 [s], 'converged' bool [s] and 'cost' float64 (s, 3) =
  {J, D, R} of the last step as numpy arrays.  NaN codes raise ValueError.
  """
  lib = vtc_hip.load_library()
  codes = _codes(codes)
  b, s = codes.shape
  device = codes.device
  host_values, host_k = _host_pair(init_codebooks)
  # fresh device copies: the fit is in place
  values, k = _device_pair((host_values, host_k), s, device)
  kmax = values.shape[1]
  zero = _on(device, cbook_inds_of_zero_pts((host_values, host_k)),
             torch.int32, (s,), 'zero_index')
  indices, _, first_status = _assign(codes, (values, k), None, 0.0, False)
  counts = index_counts(indices, kmax)
  del indices
  # the first step's input lengths, by torch (module docstring)
  lengths = -torch.log2(counts.to(torch.float64) /
                        counts.sum(1, keepdim=True).to(torch.float64))
  tensors = {
      'codebooks': values, 'lengths': lengths.contiguous(), 'counts': counts,
      'cost': torch.zeros((s, 3), dtype=torch.float64, device=device),
      'k': k, 'zero_index': zero,
      'active': torch.ones(s, dtype=torch.int32, device=device),
      'iterations': torch.zeros(s, dtype=torch.int32, device=device)}
  state = _state(tensors)
  status = torch.zeros(1, dtype=torch.int64, device=device)
  ws = vtc_hip.workspace(lib.vtc_quant_lloyd_step_workspace_bytes(b, s, kmax),
                         device)
  stream = vtc_hip.current_stream(device)
  for _ in range(int(max_iterations)):
    vtc_hip.check(lib.vtc_quant_lloyd_step(
        vtc_hip.ptr(codes), b, s, kmax, float(lagrange_mult), float(epsilon),
        1 if pin_zero else 0, ctypes.byref(state), ctypes.byref(state),
        vtc_hip.ptr(status), vtc_hip.ptr(ws), ws.numel(), stream),
                  'vtc_quant_lloyd_step')
  # the one read: everything as float64 in one buffer (module docstring)
  tail = torch.cat([tensors['active'].to(torch.float64),
                    tensors['iterations'].to(torch.float64),
                    tensors['cost'].reshape(-1),
                    (status + first_status).to(torch.float64)]).cpu().numpy()
  if tail[-1] != 0:
    raise ValueError('scalar_lloyd: the codes hold NaN')
  result = {name: tensors[name] for name in
            ('codebooks', 'k', 'lengths', 'counts', 'zero_index')}
  result['iterations'] = tail[s:2 * s].astype(np.int32)
  result['converged'] = tail[:s] == 0
  result['cost'] = tail[2 * s:5 * s].reshape(s, 3).copy()
  return result


# ------------------------------------------------------------- rate-distortion
def _reconstruct(codes, dictionary):
  """codes (b, s) @ dictionary (s, n) through vtc_fc_residual, the contraction
  of the fully-connected plugins' validation metrics, against zero images."""
  lib = vtc_hip.load_library()
  dictionary = vtc_hip.require_device_tensor(dictionary,
                                             'dictionary').contiguous()
  b, s = codes.shape
  if dictionary.dim() != 2 or dictionary.shape[0] != s:
    raise ValueError('dictionary must be (%d, n), got shape %s'
                     % (s, tuple(dictionary.shape)))
  n = dictionary.shape[1]
  zeros = torch.zeros((b, n), dtype=torch.float32, device=codes.device)
  out = torch.empty_like(zeros)
  vtc_hip.check(lib.vtc_fc_residual(
      vtc_hip.ptr(zeros), vtc_hip.ptr(dictionary), vtc_hip.ptr(codes),
      vtc_hip.ptr(out), b, n, s, vtc_hip.current_stream(codes.device)),
                'vtc_fc_residual')
  return out


def entropy_bits(counts):
  """Total bits of an ideal entropy code of each column's indices: the sum
  over the columns of -sum_i c_i log2(c_i / n), float64 on the host, from the
  (s, kmax) counts of index_counts."""
  counts = (counts.cpu().numpy() if torch.is_tensor(counts)
            else np.asarray(counts)).astype(np.float64)
  n = counts.sum(1, keepdims=True)
  with np.errstate(divide='ignore', invalid='ignore'):
    terms = np.where(counts > 0, -counts * np.log2(counts / n), 0.0)
  return float(terms.sum(1).sum())


def _distortion(patches, reconstruction, fullimg_reshape_params):
  """The distortion dictionary of compute_RD_point (its docstring)."""
  from utils import plotting
  distortion = {'pSNR': plotting.compute_pSNR(patches, reconstruction)}
  if fullimg_reshape_params is not None:
    from utils import image_processing
    dims = fullimg_reshape_params['patch_dim']
    positions = fullimg_reshape_params['patch_positions']
    original = image_processing.assemble_image_from_patches(
        patches, dims, positions)
    image = image_processing.assemble_image_from_patches(
        reconstruction, dims, positions)
    if original.shape[2] != 1:
      raise ValueError('full-image distortion is defined for one channel')
    distortion = {'pSNR_patches': distortion['pSNR'],
                  'pSNR': plotting.compute_pSNR(original[:, :, 0].contiguous(),
                                                image[:, :, 0].contiguous()),
                  'SSIM': plotting.compute_ssim(original[:, :, 0].contiguous(),
                                                image[:, :, 0].contiguous())}
  return distortion


def compute_RD_point(codes, patches, dictionary, codebooks, lengths=None,
                     lagrange_mult=0.0, source_code='jpeg', tables=None,
                     fullimg_reshape_params=None, from_stream=False,
                     rows_per_stream=None):
  """One rate-distortion point of quantised codes.

  codes : (b, s) float32 device tensor; patches : (b, n) float32 device
  tensor; dictionary : (s, n) float32 device tensor, patches ~ codes @
  dictionary.  The codes are assigned (assign, with lengths and lagrange_mult)
  and dequantised, and the patches reconstructed from the dequantised codes.

  source_code 'jpeg': the indices relative to each column's zero codeword go
  through the run-length and Huffman source code of utils.jpeg; `tables` =
  (huff_table_ac, huff_table_dc), trained on these indices when None.  A
  column without a zero codeword raises ValueError.  'entropy': the sum over
  the columns of the empirical entropy of the indices (entropy_bits); tables
  is returned as it came.  'huffman': every column's indices under a Huffman
  table of its own (utils.index_coding, include/vtc_index_code.h); `tables` is
  a list of s dicts {index: codeword}, trained on these indices when None
  (index_huffman_tables of their counts: every index below the column's k is
  codable, seen or not), and the rate is the total of index_code_bits, the
  bits a decoder would read.  With tables trained on other data this is an
  out-of-sample rate, which no entropy figure of the data itself gives.
  'ans': every column's indices under a row of range-coder frequencies
  (index_coding.index_ans_frequencies, include/vtc_index_ans.h); `tables` is
  the uint16 (s, kmax) frequency array, trained on these indices when None,
  and the rate is 8 x the total bytes of the streams of
  index_coding.index_ans_stream_bytes with `rows_per_stream` rows each (None:
  its default), the 256-byte flush of every stream included.  A prefix code
  pays at least one bit per index; this one does not.

  from_stream (source_code 'huffman' and 'ans' only, ValueError otherwise):
  the indices are packed with index_coding.pack_index_streams
  (pack_index_ans) and read back by decode_codes; reconstruction and
  distortion are those of the decoded codes and the rate is the streams' total
  bits / patches.numel().  What is charged has then been decoded, and what is
  measured has been through the bytes.

  Returns (rate in bits per pixel, distortion, tables).  distortion is
  {'pSNR': utils.plotting.compute_pSNR(patches, reconstruction)}; with
  fullimg_reshape_params = {'patch_dim', 'patch_positions'} both are
  reassembled with assemble_image_from_patches and distortion is {'pSNR',
  'SSIM'} of the images, with the patch figure under 'pSNR_patches'.
  """
  from utils import jpeg
  coder = _source_coder(source_code, from_stream, jpeg=True)
  codes = _codes(codes)
  patches = _codes(patches, 'patches')
  if patches.shape[0] != codes.shape[0]:
    raise ValueError('one patch per row of codes')
  s = codes.shape[1]
  pair = _device_pair(codebooks, s, codes.device)
  if lengths is None and isinstance(codebooks, dict):
    lengths = codebooks.get('lengths')
  if source_code == 'jpeg':
    zero = (codebooks['zero_index'].cpu().numpy()
            if isinstance(codebooks, dict) and 'zero_index' in codebooks
            else cbook_inds_of_zero_pts(pair))
    missing = np.nonzero(np.asarray(zero) < 0)[0]
    if len(missing):
      raise ValueError('column %d has no zero codeword: the JPEG source code '
                       'needs one' % missing[0])
  indices, dequantized, status = _assign(codes, pair, lengths, lagrange_mult,
                                         True)
  if not from_stream:
    reconstruction = _reconstruct(dequantized, dictionary)
  if source_code == 'jpeg':
    levels = jpeg._relative_levels(indices, zero)
    if tables is None:
      tables = jpeg.tables_from_counts(*jpeg.symbol_counts(levels))
    bits = jpeg.stream_bits(levels, tables[0], tables[1])
    total_bits = int(jpeg.bit_offsets(bits)[-1])
  elif not coder.has_tables:
    total_bits = entropy_bits(index_counts(indices, pair[0].shape[1]))
  else:
    if int(status) != 0:   # before the coder meets their index -1
      raise ValueError('compute_RD_point: the codes hold NaN')
    if tables is None:
      tables = coder.train(index_counts(indices, pair[0].shape[1]), pair[1])
    if from_stream:
      streams = coder.pack(indices, tables, rows_per_stream)
      total_bits = streams.bits
      reconstruction = _reconstruct(
          dequantize_assignments(coder.unpack(streams, tables), pair),
          dictionary)
    else:
      total_bits = coder.total_bits(indices, tables, rows_per_stream)
  if int(status) != 0:
    raise ValueError('compute_RD_point: the codes hold NaN')
  rate = total_bits / float(patches.numel())
  return rate, _distortion(patches, reconstruction,
                           fullimg_reshape_params), tables


def _source_coder(source_code, from_stream, jpeg=False, mixed=False):
  """The description of `source_code` in index_coding.SOURCE_CODES, after the
  checks every R-D entry point makes of the name: None for 'jpeg' where the
  entry point takes it (it codes levels, not indices, and has no description);
  ValueError for any other name without one and, outside the mixed points,
  for a code of a single column; ValueError for from_stream with a code that
  writes no streams of indices."""
  coder = None
  if not (jpeg and source_code == 'jpeg'):
    coder = _coding.SOURCE_CODES.get(source_code)
    if coder is None or (coder.one_column and not mixed):
      raise ValueError("source_code must be %s'entropy', 'huffman' or 'ans'"
                       % ("'jpeg', " if jpeg else ''))
  if from_stream and not (coder and coder.writes_streams):
    raise ValueError("from_stream=True needs source_code='huffman' or 'ans': "
                     'only those source codes write streams of indices')
  return coder


def _stream_set(packed, offsets, ans_shape):
  """(coder, stream set) of what the public decoders are given: Huffman
  streams, or with ans_shape = (b, rows_per_stream) those of the range
  coder."""
  if ans_shape is None:
    return _coding.Huffman, _coding.StreamSet(packed, offsets, None, None,
                                              None)
  b, rows_per_stream = ans_shape
  return _coding.Ans, _coding.StreamSet(packed, offsets, b, rows_per_stream,
                                        None)


def decode_codes(packed, offsets, tables, codebooks, ans_shape=None):
  """The (b, s) float32 dequantised codes whose index streams are in (packed,
  offsets), what index_coding.pack_index_streams returns for the (b, s)
  indices of `assign`: index_coding.unpack_index_streams under the s tables,
  then dequantize_assignments with the codebooks.  One host read (the
  decoder's status).

  ans_shape = (b, rows_per_stream): (packed, offsets) are the range-coded
  streams of index_coding.pack_index_ans instead, `tables` the uint16 (s,
  kmax) frequencies, and index_coding.unpack_index_ans reads them."""
  coder, streams = _stream_set(packed, offsets, ans_shape)
  return dequantize_assignments(coder.unpack(streams, tables), codebooks)


def _need_tables(who, coder, *tables):
  if any(table is None for table in tables):
    raise ValueError('%s: source_code=%r with precomputed codebooks needs %s '
                     'of the training call as well'
                     % (who, coder.name, coder.tables_noun))


def _uniform_for(codes, binwidths, quant_multiplier):
  from utils import plotting
  summary = plotting.code_summary(codes)
  widths = np.asarray(binwidths, dtype=np.float64) * quant_multiplier
  return uniform_codebooks(summary['min'].cpu().numpy(),
                           summary['max'].cpu().numpy(), widths)


def _tables(first, second):
  return None if first is None or second is None else (first, second)


def jpeg_compute_RD_point(codes, patches, dictionary, quant_multiplier=1.0,
                          binwidths=None, precomputed_codebook=None,
                          precomputed_huff_tab_ac=None,
                          precomputed_huff_tab_dc=None,
                          fullimg_reshape_params=None):
  """The experiment's jpeg_compute_RD_point: uniform codebooks with bins of
  binwidths * quant_multiplier over the range of the codes, the JPEG source
  code.  Training call (no precomputed_codebook): returns (rate, distortion,
  codebook, huff_table_ac, huff_table_dc), the codebook as the pair
  (codebooks, k) of uniform_codebooks.  Test call (precomputed_*): returns
  (rate, distortion), as the experiment unpacks it."""
  training = precomputed_codebook is None
  codebook = (_uniform_for(codes, binwidths, quant_multiplier) if training
              else precomputed_codebook)
  rate, distortion, tables = compute_RD_point(
      codes, patches, dictionary, codebook, source_code='jpeg',
      tables=_tables(precomputed_huff_tab_ac, precomputed_huff_tab_dc),
      fullimg_reshape_params=fullimg_reshape_params)
  if training:
    return rate, distortion, codebook, tables[0], tables[1]
  return rate, distortion


def baseline_compute_RD_point(codes, patches, dictionary, quant_multiplier=1.0,
                              binwidths=None, precomputed_codebook=None,
                              precomputed_huff_tab1=None,
                              precomputed_huff_tab2=None,
                              fullimg_reshape_params=None,
                              source_code='entropy', from_stream=False,
                              rows_per_stream=None):
  """The experiment's baseline_compute_RD_point: uniform codebooks with bins
  of binwidths * quant_multiplier.  The return slots are those of the
  experiment, (rate, distortion, codebook, huff_tab1, huff_tab2) from the
  training call and (rate, distortion) from a call with precomputed_codebook.

  source_code 'entropy' (the default): every column is coded at the empirical
  entropy of its indices.  An entropy figure needs no table, so the two table
  slots are None (and the precomputed_huff_tab* arguments are accepted and
  unused); on test data the rate is then the entropy of the test indices, not
  the cost of a code trained elsewhere.

  source_code 'huffman': every column's indices under a Huffman table of its
  own (compute_RD_point).  The experiment's missing module never said what its
  table slots held; here the training call returns huff_tab1 = the list of s
  scalar tables and huff_tab2 = None, and a test call (precomputed_codebook
  and precomputed_huff_tab1) measures the bits of the test indices under the
  trained tables.  Precomputed codebooks without the tables raise
  ValueError.  from_stream: as in compute_RD_point.

  source_code 'ans': as 'huffman' with the range coder of compute_RD_point;
  huff_tab1 is then the uint16 (s, kmax) frequency array, and rows_per_stream
  is that of compute_RD_point."""
  coder = _source_coder(source_code, from_stream)
  training = precomputed_codebook is None
  if coder.has_tables and not training:
    _need_tables('baseline_compute_RD_point', coder, precomputed_huff_tab1)
  codebook = (_uniform_for(codes, binwidths, quant_multiplier) if training
              else precomputed_codebook)
  rate, distortion, tables = compute_RD_point(
      codes, patches, dictionary, codebook, source_code=source_code,
      tables=(precomputed_huff_tab1 if coder.has_tables and not training
              else None),
      fullimg_reshape_params=fullimg_reshape_params, from_stream=from_stream,
      rows_per_stream=rows_per_stream)
  if training:
    return (rate, distortion, codebook,
            tables if coder.has_tables else None, None)
  return rate, distortion


def Mod1_compute_RD_point(codes, patches, dictionary, quant_multiplier=1.0,
                          init_binwidths=None, precomputed_codebook=None,
                          precomputed_codebook_lengths=None,
                          precomputed_huff_tab1=None,
                          fullimg_reshape_params=None, max_iterations=50,
                          epsilon=1e-5, source_code='entropy',
                          from_stream=False, rows_per_stream=None):
  """The experiment's Mod1_compute_RD_point: entropy-constrained scalar Lloyd
  quantisers (scalar_lloyd) started from uniform codebooks of bin width
  init_binwidths, with lagrange_mult = quant_multiplier; the rate is the
  empirical entropy of the indices.  Training call: returns (rate,
  distortion, codebook, codeword lengths, huff_tab1) where codebook is the
  dictionary of scalar_lloyd, the lengths its 'lengths' and the last slot,
  the experiment's Huffman table, is None (see baseline_compute_RD_point).
  Test call (precomputed_codebook and precomputed_codebook_lengths): returns
  (rate, distortion).

  With source_code='huffman' the rate is the bits of the indices under one
  Huffman table per column, huff_tab1 is the list of those s tables, and a
  test call takes them back as precomputed_huff_tab1 (ValueError without
  them), as baseline_compute_RD_point does; from_stream likewise, and
  source_code='ans' with rows_per_stream (huff_tab1 the frequency array)."""
  coder = _source_coder(source_code, from_stream)
  training = precomputed_codebook is None
  if coder.has_tables and not training:
    _need_tables('Mod1_compute_RD_point', coder, precomputed_huff_tab1)
  if training:
    fit = scalar_lloyd(codes, _uniform_for(codes, init_binwidths, 1.0),
                       lagrange_mult=quant_multiplier,
                       max_iterations=max_iterations, epsilon=epsilon)
    codebook, lengths = fit, fit['lengths']
  else:
    codebook, lengths = precomputed_codebook, precomputed_codebook_lengths
  rate, distortion, tables = compute_RD_point(
      codes, patches, dictionary, codebook, lengths=lengths,
      lagrange_mult=quant_multiplier, source_code=source_code,
      tables=(precomputed_huff_tab1 if coder.has_tables and not training
              else None),
      fullimg_reshape_params=fullimg_reshape_params, from_stream=from_stream,
      rows_per_stream=rows_per_stream)
  if training:
    return (rate, distortion, codebook, lengths,
            tables if coder.has_tables else None)
  return rate, distortion
