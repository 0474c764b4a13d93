"""Scene graphs in, pictures out: the sampling path (surface of the reference's scripts/sample_images.py and the parts of
scene_generation/data/utils.py it needs).

    python -m scene_generation_amd.sample --checkpoint CKPT.pt --output_dir OUT [--weights ema] [--scene_graphs FILE.json [--bank DIR]]
                                          [--layouts FILE.json] [--consistent_graphs 1] [--graph_metrics 1]
                                          [--sample_attributes 1 --attributes_file F.pickle [--attribute_size_rule geometric]]
                                          [--quasi_random 1 [--qmc_seed S] [--qmc_max_objects J]]

* ``Sampler``: one test-mode forward per collated batch (``sample_batch``, the flags of sample_images.py:203-221) or per list of
  scene graphs written by a person (``sample_json`` -> Model.forward_json), then the device-side ``imagenet_deprocess_batch``
  (sg_deprocess_images) straight to the uint8 (N, H, W, 3) array an image writer wants, and optionally the label-map picture
  (sg_layout_rgb).  The only host synchronisation of a call is the one ``tolist()`` of the class ids that Model.forward needs
  anyway (done here and handed to the model).  With ``factored`` the stem of the generator runs on the factored test-mode layout
  (Model.factored_test_layout) and the dense (N, num_objs + rep_size, H, W) tensor is only written when a caller asks for it.
* the box IoU bookkeeping of sample_images.py:241-255 as tensor operations (``iou_totals``), read once at the end.
* ``graph_metrics`` (off by default): how many of the call's triples and attribute bits the predicted boxes and masks honour
  (scene_generation_amd.scenegraph), accumulated on the device next to the IoU totals and read once by ``graph_summary``.
* ``sample_attributes`` (off by default; needs ``attribute_stats``, an ``attributes.AttributeStats``): the size and location blocks a
  batch or a scene graph does not give are drawn from the class statistics under the graph's relations (one launch,
  scene_generation_amd.attributes), the reference's ``--sample_attributes 1``; bits that are given are kept.
* ``accuracy`` (an ``accuracy.AccuracyMeter``, off by default): the object classifier's verdict on the crops of the generated images
  (sample_images.py:224-239), accumulated on the device and read once; ``--accuracy_model_path`` on the command line.
* ``inception`` (an ``inception.InceptionScore``, off by default): the Inception score of the generated images (train.py:177-225
  applies it to validation batches; here to whatever is sampled), softmax rows accumulated on the device and read once by
  ``inception_summary``; ``--inception_weights`` on the command line.
* ``fid`` (a ``fid.FrechetInceptionDistance``, off by default): the Frechet Inception Distance of the generated images to the real
  statistics the object holds, float64 moments accumulated on the device and read once by ``fid_summary``; ``--fid_stats`` on the
  command line.
* ``sets`` (a ``featsets.FeatureSetMetrics``, off by default): KID and precision / recall / density / coverage of the generated images
  against the real feature rows the object holds, fed from the same Inception forward as ``fid`` / ``inception`` when one of them
  carries it, read once by ``featsets_summary``; ``--real_features`` on the command line.
* ``--fid_infinity 1`` (with ``--fid_stats``) puts a ``fidinf.FIDInfinity`` in the ``sets`` slot of ``fid``, the ``FeatureSetMetrics``
  behind it (``then``): the FID extrapolated to an infinite number of images, from the same forward.
* ``--is_infinity 1`` (with ``--inception_weights``) reads an ``isinf.ISInfinity`` over the rows the scorer holds after the last batch:
  the Inception score extrapolated to an infinite number of images, from the same forward.
* ``diversity`` (an ``lpips.Diversity``, off by default): the mean LPIPS distance between two pictures of the same scene graph with
  different appearance draws.  ``sample_pair`` runs ``sample_batch`` and then a second forward of the same batch with fresh bank
  draws that feeds this scorer ONLY; read once by ``diversity_summary``; ``--diversity_backbone`` / ``--diversity_lin`` /
  ``--diversity_net`` on the command line.
* ``quasi_random`` (a ``qmc.QuasiRandomInputs``, off by default; ``--quasi_random 1 [--qmc_seed S] [--qmc_max_objects J]``): the
  k-th scored image takes its mask-noise row, its objects' bank rows and attribute uniforms from point k of a scrambled Sobol
  sequence, generated and consumed on the device (three launches in front of the forward instead of the host loop over the bank);
  the second forward of ``sample_pair`` draws from a stream of its own.  ``Sampler.last_draws`` keeps the last tables.
* ``run_model`` / the command line: load a checkpoint (``--weights model | best | ema | ema_best``), sample, write PNG files
  (PIL, imported only when a file is written; ``.npy`` when PIL is absent).
Not here: scene-graph drawing, the GUI server, the COCO loaders (``scene_generation.data`` stays the host
checkout's under install_as)."""
import argparse
import json
import os
import random

import numpy as np
import torch

from . import ops
from .evaluate import _area, intersection
from .utils import bool_flag, int_tuple, to_device_async

WEIGHT_KEYS = {'model': 'model_state', 'best': 'model_best_state', 'ema': 'model_ema_state', 'ema_best': 'model_ema_best_state'}


def imagenet_deprocess_batch(imgs, rescale=True):
    """data/utils.py:32-51 with the reference's contract -- a CPU float tensor (N, C, H, W) in [0, 255] -- computed on the device
    (ops.deprocess_images); the copy to the host is the call's synchronisation, as ``imgs.cpu()`` is the reference's."""
    return ops.deprocess_images(imgs, rescale=rescale, uint8=False, float32=True).cpu()


def iou_totals(boxes_pred, boxes_gt, obj_to_img):
    """sample_images.py:241-255 without the Python loop: an object is kept iff it is not the last of the batch and the next object
    belongs to the same image (that drops every image's trailing __image__ object).  -> float tensor [4] on the boxes' device:
    (sum of IoU, #IoU > 0.5, #IoU > 0.3, #kept) over the kept boxes (metrics.py:27-35).  No host synchronisation."""
    O = obj_to_img.numel()
    keep = torch.zeros(O, dtype=torch.bool, device=obj_to_img.device)
    if O > 1:
        keep[:-1] = obj_to_img[:-1] == obj_to_img[1:]
    inter = intersection(boxes_pred, boxes_gt)
    iou = inter / (_area(boxes_pred) + _area(boxes_gt) - inter)
    zero = torch.zeros_like(iou)
    iou = torch.where(keep, iou, zero)                      # a dropped box (possibly degenerate: NaN) counts for nothing
    return torch.stack([iou.sum(), (iou > 0.5).sum().to(iou.dtype), (iou > 0.3).sum().to(iou.dtype), keep.sum().to(iou.dtype)])


def iou_summary(totals):
    """the ONE device-to-host read of the bookkeeping: {'avg_iou', 'r0.5', 'r0.3', 'total_boxes'}"""
    s, r5, r3, n = [float(v) for v in totals.tolist()]
    return {'avg_iou': s / n if n else float('nan'), 'r0.5': r5 / n if n else float('nan'),
            'r0.3': r3 / n if n else float('nan'), 'total_boxes': int(n)}


class SampleOut(object):
    """images uint8 (N, H, W, 3); boxes_pred (O, 4); masks_pred (O, M, M); layout_rgb fp32 (N, 3, H, W) in [0, 255] or None;
    layout: the dense test-mode layout or None; objs (sample_json)"""

    def __init__(self, images, boxes_pred, masks_pred, layout_rgb=None, layout=None, objs=None):
        self.images, self.boxes_pred, self.masks_pred = images, boxes_pred, masks_pred
        self.layout_rgb, self.layout, self.objs = layout_rgb, layout, objs


class Sampler(object):
    """``features``: the appearance bank {class id: array [rows, rep_size]} that replaces the crops' encoding when a batch is
    sampled without ground-truth textures (features_clustered_001.npy of the reference).  ``colors``: [num_objs, 3] table of the
    label-map picture (default: torch.randint(0, 256), sample_images.py:197).  ``factored``: run the generator's stem on the
    factored test-mode layout (Model.factored_test_layout).  ON by default: measured on MI355X at N = 32 / 128 x 128, 6.82 against
    7.98 ms per batch with a spread of 0.17 ms between blocks; ``factored=False`` is the dense baseline.
    ``sample_attributes`` (with ``attribute_stats``): attribute blocks without a bit are drawn from the class statistics
    (attributes.sample_attributes, size rule ``attribute_size_rule``); call k of this sampler draws with seed ``attribute_seed + k``,
    so successive batches differ and a run is reproducible.  Off: nothing new is launched."""

    def __init__(self, model, features=None, colors=None, factored=True, graph_metrics=False, accuracy=None, inception=None,
                 fid=None, diversity=None, sets=None, attribute_stats=None, sample_attributes=False, attribute_seed=0,
                 attribute_size_rule='reference', quasi_random=None):
        self.quasi_random = quasi_random     # qmc.QuasiRandomInputs: one Sobol point per scored image, or None (nothing new runs)
        self._quasi_pair = None              # the stream of sample_pair's second, unscored forward (seed + 1), made on first use
        self._device_bank = None             # qmc.DeviceBank of ``features``, packed on first use
        self._pair_u = None                  # the scored forward's attribute uniforms, for the second forward of a pair
        self.last_draws = None               # (noise, pick, u, row_idx) of the last quasi-random call (tests, debugging)
        self.sample_attributes = bool(sample_attributes)
        if self.sample_attributes:
            from .attributes import SIZE_RULES
            if attribute_stats is None:
                raise ValueError('sample_attributes needs the class statistics (Sampler(attribute_stats=...) / --attributes_file)')
            if attribute_size_rule not in SIZE_RULES:
                raise ValueError('attribute_size_rule %r: expected one of %s' % (attribute_size_rule, ', '.join(SIZE_RULES)))
        self.attribute_stats, self.attribute_size_rule = attribute_stats, attribute_size_rule
        self.attribute_seed = int(attribute_seed)      # the seed of the NEXT call's table of uniforms
        self.diversity = diversity           # lpips.Diversity fed by sample_pair, or None
        self.sets = sets                     # featsets.FeatureSetMetrics whose fake side every forward feeds, or None
        self.model, self.features, self.factored = model, features, bool(factored)
        self.accuracy = accuracy             # accuracy.AccuracyMeter fed by sample_batch, or None
        self.inception = inception           # inception.InceptionScore fed by every forward, or None
        self.fid = fid                       # fid.FrechetInceptionDistance whose fake side every forward feeds, or None
        self.graph_metrics = bool(graph_metrics)
        self.graph_counts = None             # running agreement counters (scenegraph.new_counts), on the device
        self.device = next(model.parameters()).device
        if colors is None:
            colors = torch.randint(0, 256, [model.num_objs, 3]).float()
        self.colors = to_device_async(torch.as_tensor(colors, dtype=torch.float32).contiguous(), self.device)
        self.iou = None                      # running (sum IoU, > 0.5, > 0.3, boxes) of sample_batch, on the device

    # -- the forward + what follows the network -------------------------------------------------------------------------------------
    def _forward(self, fn, objs_h, o2i_h, want_layout_rgb, want_layout, objs, score=None, scored=True, noise=None):
        """``scored=False`` (the second forward of ``sample_pair``): no scorer sees the network's output.  ``noise`` [N, mask_noise_dim]
        (quasi-random inputs): the model's noise_override for this forward only."""
        m = self.model
        saved = (m.factored_test_layout, m.objs_host, m.obj_to_img_host, m.noise_override)
        m.factored_test_layout, m.objs_host, m.obj_to_img_host = self.factored, objs_h, o2i_h
        if noise is not None:
            m.noise_override = noise
        try:
            with torch.no_grad():
                imgs_pred, boxes_pred, masks_pred, _, layout, _ = fn()
                if score is not None:                       # the accuracy network reads the network's output, before deprocessing
                    score(imgs_pred, boxes_pred)
                if scored and self.inception is not None:   # likewise the Inception network (no host synchronisation)
                    self.inception(imgs_pred)
                if scored and self.fid is not None and getattr(self.inception, 'fid', None) is not self.fid:      # (else fed by the scorer's forward)
                    self.fid(imgs_pred)
                if scored and self.sets is not None and not self._sets_shared():
                    self.sets(imgs_pred)
                images = ops.deprocess_images(imgs_pred, rescale=True, uint8=True)
                rgb = None
                if want_layout_rgb:
                    planes = ops.hint(layout, 'test_planes')
                    if planes is not None:                  # factored: the winner / value planes the layout was built from
                        rgb = ops.layout_rgb(planes[0], planes[1], objs, self.colors)
                    else:   # dense baseline: a pixel's only non-zero one-hot channel is its winner's class and holds the value
                        value, cls = layout[:, :m.num_objs].max(1)
                        winner = torch.where(value > 0, cls, torch.full_like(cls, -1)).to(torch.int32)
                        table = torch.arange(m.num_objs, dtype=torch.int64, device=layout.device)
                        rgb = ops.layout_rgb(winner.contiguous(), value.contiguous(), table, self.colors)
                if want_layout:
                    ops.ensure_dense(layout)                # factored: the deferred dense kernel runs only here
        finally:
            m.factored_test_layout, m.objs_host, m.obj_to_img_host, m.noise_override = saved
        return SampleOut(images, boxes_pred, masks_pred, rgb, layout if want_layout else None, objs)

    def sample_batch(self, batch, use_gt_boxes=False, use_gt_masks=False, use_gt_textures=False, use_gt_attr=False,
                     want_layout_rgb=False, want_layout=False, _scored=True):
        """One collated batch (imgs, objs, boxes, masks, triples, obj_to_img, triple_to_img, attributes), the flags of
        sample_images.py:203-221.  Without ground-truth textures every object takes a random row of its class's bank, drawn with
        ``random.randint`` in object order like the reference (``random.seed`` reproduces it); with ``quasi_random`` the rows, the
        noise and the attribute uniforms come from the image's Sobol point instead, on the device.  (``_scored=False``, the second
        forward of ``sample_pair``: the same forward with no scorer fed and no counter touched.)"""
        imgs, objs, boxes, masks, triples, obj_to_img, triple_to_img, attributes = [t.to(self.device) for t in batch]
        objs_h, o2i_h = torch.stack((objs, obj_to_img)).tolist()        # the call's one host synchronisation
        features = None
        noise = u = None
        if self.quasi_random is not None:    # the image's noise row, bank picks and attribute uniforms from its Sobol point (qmc.py)
            noise, pick, u = self._quasi_draw(obj_to_img, imgs.size(0), o2i_h, _scored)
            row_idx = None
            if not use_gt_textures:
                features, row_idx = self._quasi_bank().draw(objs, pick, objs_host=objs_h)      # [O, rep_size], on the device
            self.last_draws = (noise, pick, u, row_idx)
            if _scored:
                self._pair_u = u
        elif not use_gt_textures:
            if self.features is None:
                raise ValueError('No features file')                    # sample_images.py:174
            rows = []
            for c in objs_h:
                bank = self.features[c]
                rows.append(bank[random.randint(0, bank.shape[0] - 1), :])
            features = list(to_device_async(torch.from_numpy(np.stack(rows).astype(np.float32)), self.device).unbind(0))
        given_attributes = attributes        # what the batch specified: the graph metrics score these
        if not use_gt_attr:
            attributes = torch.zeros_like(attributes)
        if self.sample_attributes and _scored:                          # blocks without a bit are drawn; the metrics score the result
            attributes = given_attributes = self._fill_attributes(objs, triples, obj_to_img, attributes, o2i_h, triple_to_img, u=u)
        elif self.sample_attributes:                                    # the second forward of a pair: the first one's draw again
            attributes = self._fill_attributes(objs, triples, obj_to_img, attributes, o2i_h, triple_to_img, advance=-1,
                                               u=self._pair_u if u is not None else None)
        m = self.model
        score = None
        if _scored and self.accuracy is not None:        # sample_images.py:224-239: crops at the ground-truth boxes when they drive the layout
            def score(imgs_pred, boxes_pred):
                self.accuracy.update(imgs_pred, boxes if use_gt_boxes else boxes_pred, obj_to_img, objs)
        out = self._forward(lambda: m(imgs, objs, triples, obj_to_img, boxes_gt=boxes, masks_gt=masks if use_gt_masks else None,
                                      attributes=attributes, test_mode=True, use_gt_box=use_gt_boxes, features=features),
                            objs_h, o2i_h, want_layout_rgb, want_layout, objs, score, _scored,
                            **({} if noise is None else {'noise': noise}))      # (off: the call is the one it always was)
        if not _scored:
            return out
        tot = iou_totals(out.boxes_pred, boxes, obj_to_img)
        self.iou = tot if self.iou is None else self.iou + tot
        self._graph_metrics(out, triples, given_attributes)
        return out

    def sample_pair(self, batch, use_gt_boxes=False, use_gt_masks=False, use_gt_textures=False, use_gt_attr=False,
                    want_layout_rgb=False, want_layout=False):
        """``sample_batch`` (IoU, accuracy, Inception, FID and the graph counters see this forward only), then a second forward of
        the same batch with fresh draws from the appearance bank; the two sets of pictures go to the diversity scorer as pairs (no
        host synchronisation beyond the two forwards').  -> (SampleOut, SampleOut).  With ground-truth textures nothing is random and
        both forwards give the same picture: that raises instead of reporting a diversity of 0.  (The second forward draws from
        ``random`` like any forward -- the bank rows, and the model's appearance pool -- so the stream moves on.)"""
        if self.diversity is None:
            raise ValueError('sample_pair: the sampler was built without a diversity scorer (Sampler(diversity=...))')
        if use_gt_textures:
            raise ValueError('sample_pair: with use_gt_textures nothing is random -- both forwards would give the same picture and '
                             'the diversity would be 0 by construction; diversity needs the appearance bank\'s draws')
        first = self.sample_batch(batch, use_gt_boxes, use_gt_masks, False, use_gt_attr, want_layout_rgb, want_layout)
        second = self.sample_batch(batch, use_gt_boxes, use_gt_masks, False, use_gt_attr, _scored=False)
        self.diversity(first.images, second.images)
        return first, second

    def sample_json(self, scene_graphs, want_layout_rgb=False, want_layout=False):
        """Scene graphs as dictionaries (Model.encode_scene_graphs, which APPENDS to them) -> SampleOut with ``objs``."""
        m = self.model
        if isinstance(scene_graphs, dict):
            scene_graphs = [scene_graphs]
        objs, triples, obj_to_img, attributes, features = m.encode_scene_graphs(scene_graphs)
        objs_h, o2i_h = torch.stack((objs, obj_to_img)).tolist()
        noise = u = None
        if self.quasi_random is not None:    # noise and attribute columns; the bank rows are the graphs' own feature numbers, as ever
            noise, pick, u = self._quasi_draw(obj_to_img, max(o2i_h) + 1, o2i_h, True)
            self.last_draws = (noise, pick, u, None)
        if self.sample_attributes:
            attributes = self._fill_attributes(objs, triples, obj_to_img, attributes, o2i_h, u=u)
        out = self._forward(lambda: m(None, objs, triples, obj_to_img, attributes=attributes, test_mode=True, use_gt_box=False,
                                      features=features), objs_h, o2i_h, want_layout_rgb, want_layout, objs,
                            **({} if noise is None else {'noise': noise}))
        self._graph_metrics(out, triples, attributes)
        return out

    def _fill_attributes(self, objs, triples, obj_to_img, attributes, o2i_h, triple_to_img=None, advance=0, u=None):
        """with ``sample_attributes``: one launch that draws the size / location blocks ``attributes`` leaves empty (given bits are
        kept) with the seed of this call, then moves the seed on; no host synchronisation (the host list is the call's own).
        ``advance=-1``: the previous call's seed again, and the seed stays.  ``u`` (quasi-random inputs): the device table of
        uniforms to draw with, instead of the one made on the host from the seed."""
        from .attributes import sample_attributes
        seed = self.attribute_seed + advance
        block, _, _ = sample_attributes(objs, triples, obj_to_img, self.attribute_stats, given=attributes, seed=seed, u=u,
                                        triple_to_img=triple_to_img, obj_to_img_host=o2i_h, size_rule=self.attribute_size_rule)
        self.attribute_seed = seed + 1
        return block

    def _quasi_draw(self, obj_to_img, N, o2i_h, scored):
        """(noise, pick, u) of the next N points: of the scored stream, or -- the second forward of ``sample_pair`` -- of a second
        stream with seed + 1, so that the scored one moves by one point per scored image whatever else is sampled"""
        q = self.quasi_random
        if not scored:
            if self._quasi_pair is None:
                from .qmc import QuasiRandomInputs
                self._quasi_pair = QuasiRandomInputs(q.noise_dim, q.max_objects, seed=q.seed + 1, device=self.device)
            q = self._quasi_pair
        if q.noise_dim != self.model.mask_noise_dim:
            raise ValueError('quasi_random draws noise rows of %d columns, the model\'s mask noise has %d'
                             % (q.noise_dim, self.model.mask_noise_dim))
        return q.draw(obj_to_img, ops.segment_offsets(obj_to_img, N), N, obj_to_img_host=o2i_h)

    def _quasi_bank(self):
        if self._device_bank is None:
            if self.features is None:
                raise ValueError('No features file')                    # sample_images.py:174
            from .qmc import DeviceBank
            self._device_bank = DeviceBank.from_dict(self.features, self.model.num_objs, self.device)
        return self._device_bank

    def _graph_metrics(self, out, triples, attributes):
        """with ``graph_metrics``: four launches that add to the counters (centroids of the predicted masks, triple agreement, the
        derived size / location indices, attribute agreement); no host synchronisation.  Off: nothing is launched."""
        if not self.graph_metrics:
            return
        from . import scenegraph
        if self.graph_counts is None:
            self.graph_counts = scenegraph.new_counts(self.model.num_preds, self.device)
        centers = scenegraph.object_centers(out.boxes_pred, out.masks_pred)
        scenegraph.triple_agreement(triples, out.boxes_pred, centers=centers, counts=self.graph_counts)
        if attributes is not None and attributes.dim() == 2 and attributes.size(1) == scenegraph.SIZE_LEN + scenegraph.GRID ** 2:
            scenegraph.attribute_agreement(attributes, out.boxes_pred, centers=centers, counts=self.graph_counts)

    def iou_summary(self):
        return iou_summary(self.iou) if self.iou is not None else None

    def accuracy_summary(self):
        """the ONE device-to-host read of the accuracy record (AccuracyMeter.summary); None without a meter"""
        return self.accuracy.summary() if self.accuracy is not None else None

    def inception_summary(self, splits=5):
        """the ONE device-to-host read of the Inception score over everything sampled since the scorer's ``clean()``:
        {'mean', 'std', 'images', 'splits'}; None without a scorer"""
        if self.inception is None:
            return None
        mean, std = self.inception.compute_score(splits=splits)
        return {'mean': mean, 'std': std, 'images': self.inception.count, 'splits': splits}

    def _sets_shared(self):
        """``sets`` is fed by the forward of ``fid`` (attached as its ``sets``) or of the scorer (in the place of its ``fid``)"""
        for tap in (getattr(self.fid, 'sets', None), getattr(self.inception, 'fid', None)):
            while tap is not None:                          # a tap may forward to the next one (fidinf.FIDInfinity(then=...))
                if tap is self.sets:
                    return True
                tap = getattr(tap, 'then', None)
        return False

    def featsets_summary(self):
        """``FeatureSetMetrics.compute()`` over everything sampled since its ``clean()``: KID mean / std, precision, recall, density,
        coverage and the row counts; None without one"""
        return None if self.sets is None else self.sets.compute()

    def fid_summary(self):
        """the Frechet Inception Distance of everything sampled since the FID's ``clean()`` (one finalize launch, one device-to-host
        copy, the eigen-decompositions on the host): {'fid', 'images'}; None without one"""
        if self.fid is None:
            return None
        return {'fid': self.fid.compute(), 'images': self.fid.fake.count}

    def diversity_summary(self):
        """the ONE device-to-host read of the diversity scorer (lpips.Diversity.compute): {'mean', 'std', 'pairs'}; None without one"""
        return self.diversity.compute() if self.diversity is not None else None

    def graph_summary(self):
        """the ONE device-to-host read of the graph metrics (scenegraph.summary); None when they are off or nothing was sampled"""
        if self.graph_counts is None:
            return None
        from . import scenegraph
        return scenegraph.summary(self.graph_counts, self.model.vocab)


# ---- checkpoint -> model ------------------------------------------------------------------------------------------------------
def select_weights(checkpoint, which='model'):
    """the state dict ``--weights`` names: model -> model_state, best -> model_best_state, ema -> model_ema_state,
    ema_best -> model_ema_best_state"""
    if which not in WEIGHT_KEYS:
        raise ValueError('--weights %r: expected one of %s' % (which, ', '.join(sorted(WEIGHT_KEYS))))
    key = WEIGHT_KEYS[which]
    if checkpoint.get(key) is None:
        if which.startswith('ema'):
            raise ValueError('--weights %s: the checkpoint has no %s -- it was written without a generator EMA '
                             '(train with Trainer(ema_decay=...) / SG_G_EMA_DECAY)' % (which, key))
        raise ValueError('--weights %s: the checkpoint has no %s' % (which, key))
    return checkpoint[key]


def build_model(args, checkpoint, device='cuda'):
    """sample_images.py:133-144 plus the choice of weights"""
    from .model import Model
    model = Model(**checkpoint['model_kwargs'])
    model.load_state_dict(select_weights(checkpoint, getattr(args, 'weights', 'model')))
    if getattr(args, 'model_mode', 'eval') == 'eval':
        model.eval()
    else:
        model.train()
    if getattr(args, 'image_size', None):
        model.image_size = tuple(args.image_size)
    return model.to(device)


def synthetic_loader(model, batch_size, num_samples, mask_size=32, seed=0):
    """collated batches of the synthetic generator (scene_generation_amd.synthetic) shaped for ``model``"""
    from .synthetic import make_batch
    done, k = 0, 0
    while done < num_samples:
        n = min(batch_size, num_samples - done)
        yield make_batch(N=n, size=model.image_size[0], mask_size=mask_size, num_objs=model.num_objs, num_preds=model.num_preds,
                         num_attributes=model.vocab.get('num_attributes', 35), seed=seed + k)
        done, k = done + n, k + 1


def write_image(path_stem, array):
    """uint8 (H, W, 3) -> path_stem + '.png' through PIL, or '.npy' when PIL is absent; -> the path written"""
    array = np.ascontiguousarray(array)
    try:
        from PIL import Image
    except ImportError:
        np.save(path_stem + '.npy', array)
        return path_stem + '.npy'
    Image.fromarray(array).save(path_stem + '.png')
    return path_stem + '.png'


def _float_picture(chw):
    """fp32 (3, H, W) in [0, 255] -> uint8 (H, W, 3), the rounding of sg_deprocess_images"""
    a = np.nan_to_num(np.asarray(chw, dtype=np.float32), nan=0.0).transpose(1, 2, 0)
    return (np.clip(a, 0, 255) + 0.5).astype(np.uint8)


def _makedir(base, name, flag=True):
    if not flag:
        return None
    d = os.path.join(base, name)
    os.makedirs(d, exist_ok=True)
    return d


def load_scene_graphs(path):
    """a JSON file with one scene graph or a list of them; the keys encode_scene_graphs insists on get neutral defaults
    (feature number -1 = the class's single-row bank, no size / location attributes)"""
    with open(path) as f:
        sgs = json.load(f)
    sgs = [sgs] if isinstance(sgs, dict) else list(sgs)
    for sg in sgs:
        sg.setdefault('relationships', [])
        sg.setdefault('features', [-1] * len(sg['objects']))
        sg.setdefault('image_id', -1)
        sg.setdefault('attributes', {})
        sg['attributes'].setdefault('size', [])
        sg['attributes'].setdefault('location', [])
    return sgs


def load_layouts(path):
    """a JSON file with one layout of a drawing front end or a list of them (scenegraph.layout_json_to_scene_graphs) -> scene graphs"""
    from .scenegraph import layout_json_to_scene_graphs
    with open(path) as f:
        return layout_json_to_scene_graphs(json.load(f))


def load_features(args):
    """the appearance bank next to the checkpoint (sample_images.py:166-174) or ``--features``"""
    path = getattr(args, 'features', None) or os.path.join(os.path.dirname(args.checkpoint or ''), 'features_clustered_001.npy')
    if not os.path.isfile(path):
        raise ValueError('No features file')
    return np.load(path, allow_pickle=True).item()


def load_bank(directory):
    """(features_clustered_100.npy, features_clustered_001.npy) of ``directory``: the two banks scripts/gui/model.py:47-55 hangs on
    the model (``Model.features`` / ``Model.features_one``), as python -m scene_generation_amd.bank writes them"""
    banks = []
    for name in ('features_clustered_100.npy', 'features_clustered_001.npy'):
        path = os.path.join(directory, name)
        if not os.path.isfile(path):
            raise ValueError('No features file: %s' % path)
        banks.append(np.load(path, allow_pickle=True).item())
    return tuple(banks)


def run_model(args, checkpoint, output_dir, loader=None, device='cuda'):
    """sample_images.py:163-295 without COCO: sample every batch of ``loader`` (any iterable of collated batches; the synthetic
    generator when None) or the scene graphs of ``args.scene_graphs``, write one picture per image into output_dir/images
    (+ images_gt, layouts), print and return the IoU summary and the paths written."""
    if getattr(args, 'real_features', None) is not None and getattr(args, 'inception_weights', None) is None:      # before any work
        raise ValueError('--real_features needs --inception_weights (the network whose features the rows are)')
    want_attr = bool(getattr(args, 'sample_attributes', False))
    if want_attr and not getattr(args, 'attributes_file', None):
        raise ValueError('--sample_attributes 1 needs --attributes_file (python -m scene_generation_amd.attributes build, or the '
                         'reference\'s attributes_10_25.pickle)')
    want_inf = bool(getattr(args, 'fid_infinity', False))
    if want_inf and getattr(args, 'fid_stats', None) is None:
        raise ValueError('--fid_infinity needs --fid_stats (the real statistics the extrapolated distance is measured to)')
    if want_inf and loader is None and not getattr(args, 'scene_graphs', None) and not getattr(args, 'layouts', None):
        from .fidinf import check_count
        check_count(args.num_samples)       # the synthetic generator makes exactly this many: too few or too many are refused here
    want_isinf = bool(getattr(args, 'is_infinity', False))
    if want_isinf and getattr(args, 'inception_weights', None) is None:
        raise ValueError('--is_infinity needs --inception_weights (the network whose softmax rows the score is extrapolated from)')
    if want_isinf and loader is None and not getattr(args, 'scene_graphs', None) and not getattr(args, 'layouts', None):
        from .isinf import check_count as check_rows
        check_rows(args.num_samples)        # likewise: a count that gives no two subset sizes is refused before the first picture
    model = build_model(args, checkpoint, device)
    graphs = getattr(args, 'scene_graphs', None)
    layouts = getattr(args, 'layouts', None)
    if graphs and layouts:
        raise ValueError('--scene_graphs and --layouts: give one of them')
    metrics = bool(getattr(args, 'graph_metrics', False))
    stats = None
    if want_attr:
        from .attributes import AttributeStats
        stats = AttributeStats.load(args.attributes_file, model.vocab, device=device, num_classes=model.num_objs)
    if getattr(args, 'consistent_graphs', False) and model.num_preds < 7:
        raise ValueError('--consistent_graphs derives the six geometric predicates; the checkpoint knows %d' % model.num_preds)
    features = None
    if not graphs and not layouts and not args.use_gt_textures:
        features = load_features(args)
    meter = None
    acc_path = getattr(args, 'accuracy_model_path', None)
    if acc_path is not None and os.path.isfile(acc_path):      # sample_images.py:181
        from .accuracy import AccuracyMeter, load_model
        meter = AccuracyMeter(load_model(acc_path, getattr(args, 'accuracy_model_name', 'resnet101'), n_class=None, device=device),
                              input_shape=getattr(args, 'accuracy_input_shape', 224))
    scorer = None
    inc_path = getattr(args, 'inception_weights', None)
    if inc_path is not None:
        from .inception import InceptionScore
    fid, fid_inf, fid_stats = None, None, getattr(args, 'fid_stats', None)
    sets, real_features = None, getattr(args, 'real_features', None)
    if fid_stats is not None or real_features is not None:
        if inc_path is None:
            raise ValueError('--fid_stats needs --inception_weights (the network whose features the statistics are of)')
        from .inception import load_inception
        net = load_inception(inc_path, device)              # one network, one forward per batch, for every number
        if real_features is not None:
            from .featsets import FeatureSetMetrics
            sets = FeatureSetMetrics(weights=net, real_features=real_features, resize=True, batch_size=args.batch_size, device=device)
        if fid_stats is not None:
            from .fid import FrechetInceptionDistance
            attached = sets
            if want_inf:                                    # in the sets slot, the FeatureSetMetrics (if any) behind it: still one forward
                from .fidinf import FIDInfinity
                attached = fid_inf = FIDInfinity(real_stats=fid_stats, dim=net.fc.in_features, device=device, then=sets)
            fid = FrechetInceptionDistance(weights=net, real_stats=fid_stats, resize=True, batch_size=args.batch_size, device=device,
                                           sets=attached)
        # (without --fid_stats the feature rows go straight from the scorer's forward to the sets object: the same add_features)
        scorer = InceptionScore(batch_size=args.batch_size, resize=True, weights=net, device=device, fid=fid if fid is not None else sets)
    elif inc_path is not None:
        scorer = InceptionScore(batch_size=args.batch_size, resize=True, weights=inc_path, device=device)
    diversity, div_backbone, div_lin = None, getattr(args, 'diversity_backbone', None), getattr(args, 'diversity_lin', None)
    if div_backbone is not None or div_lin is not None:
        if graphs or layouts or args.use_gt_textures:
            raise ValueError('--diversity_backbone / --diversity_lin: diversity compares two appearance draws of a collated batch; '
                             'it needs the bank (no --use_gt_textures, --scene_graphs or --layouts)')
        from .lpips import LPIPS, Diversity
        diversity = Diversity(LPIPS(getattr(args, 'diversity_net', 'alex'), backbone_weights=div_backbone, lin_weights=div_lin,
                                    device=device), batch_size=args.batch_size)
    quasi = None
    if getattr(args, 'quasi_random', False):
        from .qmc import QuasiRandomInputs
        quasi = QuasiRandomInputs(model.mask_noise_dim, max_objects=getattr(args, 'qmc_max_objects', 32),
                                  seed=getattr(args, 'qmc_seed', 0), device=device)
    sampler = Sampler(model, features=features, factored=getattr(args, 'factored', True), graph_metrics=metrics, accuracy=meter,
                      inception=scorer, fid=fid, diversity=diversity, sets=sets, attribute_stats=stats, sample_attributes=want_attr,
                      attribute_seed=getattr(args, 'attribute_seed', 0),
                      attribute_size_rule=getattr(args, 'attribute_size_rule', 'reference'), quasi_random=quasi)
    img_dir = _makedir(output_dir, 'images')
    gt_dir = _makedir(output_dir, 'images_gt', args.save_gt_imgs and not graphs and not layouts)
    layout_dir = _makedir(output_dir, 'layouts', args.save_layout)
    paths, idx = [], 0

    def save(out, imgs_gt):
        nonlocal idx
        images = out.images.cpu().numpy()
        rgb = out.layout_rgb.cpu().numpy() if out.layout_rgb is not None else None
        for i in range(images.shape[0]):
            stem = '%04d' % idx
            if gt_dir is not None and imgs_gt is not None:
                write_image(os.path.join(gt_dir, stem), imgs_gt[i])
            if layout_dir is not None:
                write_image(os.path.join(layout_dir, stem), _float_picture(rgb[i]))
            paths.append(write_image(os.path.join(img_dir, stem), images[i]))
            idx += 1
        print('Saved %d images' % idx)

    if graphs or layouts:
        if getattr(args, 'features', None):
            bank = np.load(args.features, allow_pickle=True).item()
            model.features = bank
            model.features_one = bank
        if getattr(args, 'bank', None):
            model.features, model.features_one = load_bank(args.bank)
        sgs = load_scene_graphs(graphs) if graphs else load_layouts(layouts)
        if want_inf:                        # (the count is known only now: still before the first picture)
            from .fidinf import check_count
            check_count(len(sgs))
        if want_isinf:
            from .isinf import check_count as check_rows
            check_rows(len(sgs))
        for a in range(0, len(sgs), args.batch_size):
            save(sampler.sample_json(sgs[a:a + args.batch_size], want_layout_rgb=args.save_layout), None)
    else:
        if loader is None:
            loader = synthetic_loader(model, args.batch_size, args.num_samples, checkpoint['model_kwargs'].get('mask_size', 32))
            if getattr(args, 'consistent_graphs', False):   # every batch's graph re-derived from its own boxes and masks
                from .scenegraph import regraph
                loader = (regraph(batch, seed=k) for k, batch in enumerate(loader))
        for batch in loader:
            imgs_gt = None
            if gt_dir is not None:
                imgs_gt = ops.deprocess_images(batch[0].to(sampler.device), rescale=True, uint8=True).cpu().numpy()
            if diversity is not None:
                save(sampler.sample_pair(batch, args.use_gt_boxes, args.use_gt_masks, args.use_gt_textures, args.use_gt_attr,
                                         want_layout_rgb=args.save_layout)[0], imgs_gt)
                continue
            save(sampler.sample_batch(batch, args.use_gt_boxes, args.use_gt_masks, args.use_gt_textures, args.use_gt_attr,
                                      want_layout_rgb=args.save_layout), imgs_gt)
    summary = sampler.iou_summary()
    if summary is not None:
        print('avg_iou {}'.format(summary['avg_iou']))
        print('r0.5 {}'.format(summary['r0.5']))
        print('r0.3 {}'.format(summary['r0.3']))
    result = {'paths': paths, 'iou': summary}
    if meter is not None and meter.acc is not None:
        result['accuracy'] = meter.summary()
        print('Accuracy {}'.format(result['accuracy']['accuracy']))
    if scorer is not None:
        result['inception'] = sampler.inception_summary(getattr(args, 'inception_splits', 5))
        print('Inception {} {}'.format(result['inception']['mean'], result['inception']['std']))
        if want_isinf:
            from .isinf import ISInfinity
            result['is_inf'] = ISInfinity(scorer).compute()
            print('IS_inf {}'.format(result['is_inf']['is_inf']))
    if fid is not None:
        result['fid'] = sampler.fid_summary()
        print('FID {}'.format(result['fid']['fid']))
    if fid_inf is not None:
        result['fid_inf'] = fid_inf.compute()
        print('FID_inf {}'.format(result['fid_inf']['fid_inf']))
    if sets is not None:
        from .featsets import format_lines
        result['featsets'] = sampler.featsets_summary()
        for line in format_lines(result['featsets']):
            print(line)
    if diversity is not None:
        result['diversity'] = sampler.diversity_summary()
        print('Diversity {} {}'.format(result['diversity']['mean'], result['diversity']['std']))
    if metrics:
        graph = result['graph'] = sampler.graph_summary()
        if graph is not None:
            print('rel_acc {}'.format(graph['rel_acc']))
            for name, (agree, seen) in graph['rel_acc_by_pred'].items():
                print('  {}: {} / {}'.format(name, agree, seen))
            print('size_acc {}'.format(graph['size_acc']))
            print('loc_acc {}'.format(graph['loc_acc']))
    return result


def make_parser():
    p = argparse.ArgumentParser(prog='python -m scene_generation_amd.sample', description=__doc__.split('\n')[0])
    p.add_argument('--checkpoint', required=True)
    p.add_argument('--output_dir', default='output')
    p.add_argument('--weights', default='model', choices=sorted(WEIGHT_KEYS),
                   help='model_state / model_best_state / model_ema_state / model_ema_best_state of the checkpoint')
    p.add_argument('--model_mode', default='eval', choices=['train', 'eval'])
    p.add_argument('--image_size', default=None, type=int_tuple, help='default: the size the checkpoint was trained at')
    p.add_argument('--batch_size', default=24, type=int)
    p.add_argument('--num_samples', default=24, type=int, help='images from the synthetic generator when no loader is given')
    p.add_argument('--scene_graphs', default=None, help='JSON file with one scene graph or a list of them')
    p.add_argument('--features', default=None, help='appearance bank (.npy); default: features_clustered_001.npy next to the checkpoint')
    p.add_argument('--bank', default=None, help='with --scene_graphs: directory of features_clustered_100.npy (feature numbers '
                   '>= 0) and features_clustered_001.npy (feature number -1), as python -m scene_generation_amd.bank writes them')
    for flag in ('save_gt_imgs', 'use_gt_boxes', 'use_gt_masks', 'use_gt_attr', 'use_gt_textures', 'save_layout'):
        p.add_argument('--' + flag, default=False, type=bool_flag)
    p.add_argument('--factored', default=True, type=bool_flag, help='0: the dense test-mode layout (the baseline path)')
    p.add_argument('--layouts', default=None, help='JSON file with one layout or a list of them (objects with text / left / top / '
                   'width / height / size / location / feature): converted to scene graphs, then as --scene_graphs')
    p.add_argument('--consistent_graphs', default=False, type=bool_flag, help='synthetic batches: triples and attributes derived '
                   'from the batch\'s own boxes and masks instead of drawn at random')
    p.add_argument('--graph_metrics', default=False, type=bool_flag, help='report how many of the requested relations and size / '
                   'location attributes the predicted layout honours')
    p.add_argument('--sample_attributes', default=False, type=bool_flag, help='draw the size / location attributes a batch or a scene '
                   'graph does not give from the class statistics of --attributes_file, under the graph\'s relations')
    p.add_argument('--attributes_file', default=None, help='.pickle in the reference\'s format (attributes_10_25.pickle) or .npz, as '
                   'python -m scene_generation_amd.attributes build writes them')
    p.add_argument('--attribute_size_rule', default='reference', choices=['reference', 'geometric'], help='how "inside" / '
                   '"surrounding" adjust a sampled size: as the reference does, or so that the surrounding object is the larger one')
    p.add_argument('--attribute_seed', default=0, type=int, help='seed of the first batch\'s attribute draws; batch k uses seed + k')
    p.add_argument('--quasi_random', default=False, type=bool_flag, help='draw every image\'s mask noise, appearance-bank rows and '
                   'attribute uniforms from one point of a scrambled Sobol sequence, on the device (python -m pydoc '
                   'scene_generation_amd.qmc): the same --qmc_seed gives the same pictures')
    p.add_argument('--qmc_seed', default=0, type=int, help='seed of the Sobol sequence\'s scrambling')
    p.add_argument('--qmc_max_objects', default=32, type=int, help='objects per image a point holds draws for (three dimensions '
                   'each); an image with more raises')
    p.add_argument('--accuracy_model_path', default=None, help='the object classifier (python -m scene_generation_amd.accuracy '
                   'train, or the reference\'s resnet101_172_classes.pth): prints the Accuracy line of sample_images.py')
    p.add_argument('--accuracy_model_name', default='resnet101', help='its architecture: resnet18 / 34 / 50 / 101 / 152')
    p.add_argument('--accuracy_input_shape', default=224, type=int, help='side of the crops the classifier sees')
    p.add_argument('--inception_weights', default=None, help='state_dict file of torchvision\'s inception_v3 (never downloaded): '
                   'prints one "Inception MEAN STD" line over the sampled images (python -m scene_generation_amd.inception scores a '
                   'directory of images)')
    p.add_argument('--fid_stats', default=None, help='.npz with mu and sigma of the real images (python -m scene_generation_amd.fid '
                   '--save_stats, or a pytorch-fid statistics file): prints one "FID x" line; needs --inception_weights, and only the '
                   'pt_inception weights give numbers comparable with published ones')
    p.add_argument('--real_features', default=None, help='.npy with the pooled Inception features of the real images (python -m '
                   'scene_generation_amd.fid --save_features, or python -m scene_generation_amd.featsets --save_real): prints "KID mean '
                   'std", "Precision p Recall r" and "Density d Coverage c" lines; needs --inception_weights; with or without --fid_stats')
    p.add_argument('--fid_infinity', default=False, type=bool_flag, help='with --fid_stats: also print one "FID_inf x" line after the '
                   'FID line, the distance extrapolated to an infinite number of sampled images (python -m scene_generation_amd.fidinf; '
                   'at most 4096 images)')
    p.add_argument('--is_infinity', default=False, type=bool_flag, help='with --inception_weights: also print one "IS_inf x" line after '
                   'the Inception line, the score extrapolated to an infinite number of sampled images (python -m '
                   'scene_generation_amd.isinf)')
    p.add_argument('--diversity_backbone', default=None, help='torchvision alexnet / vgg16 state_dict file (never downloaded): every '
                   'batch is sampled twice with different appearance draws and one "Diversity MEAN STD" line (mean LPIPS distance '
                   'of the pairs) is printed; python -m scene_generation_amd.lpips scores two directories of pictures')
    p.add_argument('--diversity_lin', default=None, help='the LPIPS lin weights of --diversity_net (or a whole LPIPS module\'s '
                   'state_dict, which also holds the backbone); without them the unweighted baseline runs')
    p.add_argument('--diversity_net', default='alex', choices=['alex', 'vgg'])
    p.add_argument('--inception_splits', default=5, type=int, help='splits of the Inception score (train.py uses 5)')
    return p


def main(argv=None):
    args = make_parser().parse_args(argv)
    checkpoint = torch.load(args.checkpoint, map_location='cpu', weights_only=False)
    print('Loading model from ', args.checkpoint)
    return run_model(args, checkpoint, args.output_dir)


if __name__ == '__main__':
    main()
