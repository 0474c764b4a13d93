"""The Frechet Inception Distance's own operators (csrc/fid.hip, and the two pools of the FID form of the network in
csrc/inception.hip): the float64 moment update on the f64 matrix cores, its finalize, the count_include_pad=False 3x3 average pool and
the padded 3x3 stride-1 max-pool.  No wrapper synchronises.  (Part of scene_generation_amd.ops: see ops/__init__.py.)"""
import ctypes

import torch

from ._core import _call, _dev, _f32, _p, _stream

_PD = ctypes.POINTER(ctypes.c_double)


def _pd(t):
    """a float64 tensor's address as the ``double*`` the parsed prototypes ask for"""
    return ctypes.cast(t.data_ptr(), _PD)


def _moments(sum, outer, who):
    _dev(sum, who + ' sum')
    _dev(outer, who + ' outer')
    if (sum.dtype != torch.float64 or outer.dtype != torch.float64 or sum.dim() != 1 or outer.dim() != 2
            or tuple(outer.shape) != (sum.numel(), sum.numel()) or not sum.is_contiguous() or not outer.is_contiguous()
            or sum.device != outer.device):
        raise ValueError('%s: sum [D] and outer [D, D] must be contiguous float64 tensors of one device, got %s %s and %s %s'
                         % (who, sum.dtype, tuple(sum.shape), outer.dtype, tuple(outer.shape)))
    return sum.numel()


def fid_moments_update(x, sum, outer):
    """sum[j] += sum_k x[k][j]; outer[i][j] += sum_k x[k][i] x[k][j] for i <= j (the lower triangle of ``outer`` is unspecified until
    ``fid_moments_finalize``).  ``x`` float32 [rows, D], its rows contiguous (a row stride >= D is taken as it is); ``sum`` [D] and
    ``outer`` [D, D] float64, updated in place."""
    D = _moments(sum, outer, 'fid_moments_update')
    _dev(x, 'features')
    if x.dtype != torch.float32:
        raise TypeError('features must be float32, got %s' % x.dtype)
    if x.dim() != 2 or x.size(1) != D or x.device != sum.device:
        raise ValueError('fid_moments_update: x [rows, %d] on %s, got %s on %s' % (D, sum.device, tuple(x.shape), x.device))
    rows = x.size(0)
    if (D > 1 and x.stride(1) != 1) or (rows > 1 and x.stride(0) < D):
        x = x.contiguous()
    ldx = x.stride(0) if rows > 1 else D                     # (one row: the stride is never used)
    _call('sg_fid_moments_update', _p(x), rows, D, ldx, _pd(sum), _pd(outer), _stream())


def fid_moments_finalize(sum, outer, n, out=None):
    """-> (mu [D], sigma [D, D]) float64 on the device: ``sum / n`` and numpy.cov(rowvar=False) (ddof = 1) of the ``n`` rows the
    moments hold; sigma is the full matrix and equals its transpose bit for bit.  ``out``: a contiguous float64 device buffer of
    D + D * D elements the two results are views of (one device-to-host copy then moves both); a fresh one when None."""
    D = _moments(sum, outer, 'fid_moments_finalize')
    if out is None:
        out = torch.empty(D + D * D, dtype=torch.float64, device=sum.device)
    elif (out.dtype != torch.float64 or out.dim() != 1 or out.numel() != D + D * D or not out.is_contiguous()
          or out.device != sum.device):
        raise ValueError('fid_moments_finalize: out must be a contiguous float64 buffer of %d elements on %s' % (D + D * D, sum.device))
    mu, sigma = out[:D], out[D:].view(D, D)
    _call('sg_fid_moments_finalize', _pd(sum), _pd(outer), int(n), D, _pd(mu), _pd(sigma), _stream())
    return mu, sigma


def avgpool3s1x(x):
    """avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False): the divisor is the number of taps inside the plane"""
    x = _f32(x, 'avg-pool input')
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    _call('sg_avgpool3s1x_fwd', _p(x), _p(y), N * C, H, W, _stream())
    return y


def maxpool3s1(x):
    """max_pool2d(x, 3, stride=1, padding=1); a NaN in a window wins"""
    x = _f32(x, 'max-pool input')
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    _call('sg_maxpool3s1_fwd', _p(x), _p(y), N * C, H, W, _stream())
    return y
