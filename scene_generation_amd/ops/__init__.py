"""Autograd operators over the C ABI of libsg2im_hip.so (include/sg2im_hip.h).

PyTorch-ROCm is used here as plumbing only: device allocation (torch.empty), the autograd tape and the current HIP stream.
Every forward / backward is one or a few hand-written gfx950 kernel launches through ctypes; there is no eager / CPU fallback --
a CPU tensor raises.

One namespace, eighteen modules (the single 1 741-line ops.py of rounds 1-3, split by operator family in round 4):
  _core    ctypes call helpers, stream handle, workspace, parameter-gradient sinks (GradOut), path switches, layout hints,
           flat-buffer updates (Adam, fill, fold), profiler front end
  conv     Conv2d / ConvTranspose2d / sub-pixel up-conv / Linear (implicit GEMM, Winograd, head, skinny kernels)
  nn       activations, residual add, dropout mask, Instance / BatchNorm, pooling, padding
  graph    CSR build, row gather, bit-exact triple pool, embeddings, concat
  layout   masks_to_layout (dense / deferred / test mode / factored), per-image-weight convs, bilinear crops, VectorPool
           and the sampling tail (factored test-mode planes, deprocess_images, layout_rgb)
  losses   scalar losses, weighted sum, cross-entropy
  kmeans   segmented k-means of the appearance bank (assign / update / relocate / k-means++ round)
  scenegraph  scene graphs from layouts: mask centroids, attribute bits, geometric predicates, partner draw, agreement counters
  classifier  the accuracy network's own operators: padded 3x3 stride-2 max-pool, relu(a + b), BatchNorm fold, SGD step, accuracy record
  inception   the Inception score's own operators: rectangular conv into a channel slice, unpadded max-pool, count_include_pad average
              pool, bilinear resize, softmax rows, the score
  fid         the Frechet Inception Distance's own operators: the float64 moment update (f64 matrix cores) and its finalize, the two
              branch pools of the FID form of the network
  lpips       the diversity score's own operators: the wide (up to 11 x 11, stride <= 4) convolution, the scaling layer of LPIPS, one tap
              of its distance; for LPIPS as a loss the tap's gradient, the scaling layer's backward and the autograd functions
  featsets    statistics of all pairs of feature rows on the f64 matrix cores: the KID kernel sums, the k-NN manifold radii and the
              membership pass of precision / recall and density / coverage
  imageprep   Pillow's uint8 resize (bilinear / bicubic), bit for bit, over a ragged batch of packed RGB images, the loader's
              normalisation fused in
  fidinf      FID-infinity's own operators: the two Gram matrices of the shifted fake rows (f64 matrix cores) and the per-subset terms
  attributes  size and location attributes from class statistics: the per-class histogram and the relation-constrained draw
  isinf       IS-infinity's own operators: the per-row sums and entropies of the softmax rows, the score of every subset of them
  qmc         quasi-random inputs of the generator: Sobol points, their unpacking into noise / bank picks / uniforms, the bank draw
Everything is re-exported here, so ``ops.conv2d``, ``ops.GradOut``, ``ops._call`` ... keep working.  The path switches
(``ops.WINOGRAD``, ``ops.FACTORED_LAYOUT``, ``ops.UPCONV``, ``ops.HEADCONV``, ``ops.WINOGRAD24``, ``ops.COND_FOLD``) are WRITABLE through this
namespace: assigning ``ops.WINOGRAD = False`` updates the value the operator modules read (``_core.WINOGRAD``).
"""
import sys
import types

from . import _core, graph, losses, layout, conv, nn, kmeans, scenegraph, classifier, inception, fid, lpips, featsets, imageprep, fidinf, attributes, isinf, qmc

_MODULES = (_core, graph, losses, layout, conv, nn, kmeans, scenegraph, classifier, inception, fid, lpips, featsets, imageprep, fidinf, attributes,
            isinf, qmc)
_FLAGS = ('HEADCONV', 'WINOGRAD', 'WINOGRAD24', 'FACTORED_LAYOUT', 'UPCONV', 'COND_FOLD')

for _m in _MODULES:
    for _k, _v in vars(_m).items():
        if not _k.startswith('__') and not isinstance(_v, types.ModuleType):
            globals()[_k] = _v
del _m, _k, _v


class _OpsNamespace(types.ModuleType):
    def __setattr__(self, name, value):
        if name in _FLAGS:
            setattr(_core, name, value)                   # what the operator modules read
        elif name == '_call':
            for m in _MODULES:                            # tools/step_shapes.py wraps the ABI call: every module must see it
                if '_call' in vars(m):
                    setattr(m, '_call', value)
        super().__setattr__(name, value)


sys.modules[__name__].__class__ = _OpsNamespace
