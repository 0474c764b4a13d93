"""Scene graph -> image generator (surface of /root/reference/scene_generation/model.py:12-172, training branch).

Differences from the reference are confined to how the work is issued:
  * every operator is a HIP launch (scene_generation_amd.ops); no ``.item()``/``.nonzero()`` host syncs except
    the single small D2H copy of the class ids inside VectorPool.query (utils.py)
  * ``gt_layout``/``wrong_layout`` tell the layout kernel that the first ``num_objs`` channels are the constant
    one-hot block, so its backward only touches the ``rep_size`` appearance channels (model.py:165-168)
"""
import torch
import torch.nn as nn

from . import ops, streams
from .bilinear import crop_bbox_batch
from .generators import mask_net, AppearanceEncoder, define_G
from .graph import GraphTripleConv, GraphTripleConvNet
from .layers import build_mlp, Embedding, Linear
from .layout import masks_to_layout
from .utils import VectorPool, active_layout_channels, to_device_async


class Model(nn.Module):
    def __init__(self, vocab, image_size=(64, 64), embedding_dim=128, gconv_dim=128, gconv_hidden_dim=512,
                 gconv_pooling='avg', gconv_num_layers=5, mask_size=32, mlp_normalization='none',
                 appearance_normalization='', activation='', n_downsample_global=4, box_dim=128,
                 use_attributes=False, box_noise_dim=64, mask_noise_dim=64, pool_size=100, rep_size=32,
                 ngf=64, n_blocks_global=9):
        super().__init__()
        self.vocab = vocab
        self.image_size = image_size
        self.use_attributes = use_attributes
        self.box_noise_dim = box_noise_dim
        self.mask_noise_dim = mask_noise_dim
        self.object_size = 64
        self.fake_pool = VectorPool(pool_size)

        self.num_objs = len(vocab['object_to_idx'])
        self.num_preds = len(vocab['pred_idx_to_name'])
        self.obj_embeddings = Embedding(self.num_objs, embedding_dim)
        self.pred_embeddings = Embedding(self.num_preds, embedding_dim)

        attributes_dim = vocab['num_attributes'] if use_attributes else 0
        if gconv_num_layers == 0:
            self.gconv = Linear(embedding_dim, gconv_dim)
        elif gconv_num_layers > 0:
            self.gconv = GraphTripleConv(input_dim=embedding_dim, attributes_dim=attributes_dim, output_dim=gconv_dim,
                                         hidden_dim=gconv_hidden_dim, pooling=gconv_pooling,
                                         mlp_normalization=mlp_normalization)
        self.gconv_net = None
        if gconv_num_layers > 1:
            self.gconv_net = GraphTripleConvNet(input_dim=gconv_dim, hidden_dim=gconv_hidden_dim,
                                                pooling=gconv_pooling, num_layers=gconv_num_layers - 1,
                                                mlp_normalization=mlp_normalization)

        self.box_dim = box_dim
        self.box_net = build_mlp([self.box_dim, gconv_hidden_dim, 4], batch_norm=mlp_normalization)

        self.g_mask_dim = gconv_dim + mask_noise_dim
        self.mask_net = mask_net(self.g_mask_dim, mask_size)

        self.repr_input = self.g_mask_dim
        self.repr_net = build_mlp([self.repr_input, 64, rep_size], batch_norm=mlp_normalization)

        self.image_encoder = AppearanceEncoder(vocab=vocab, arch='C4-64-2,C4-128-2,C4-256-2',
                                               normalization=appearance_normalization, activation=activation,
                                               padding='valid', vecs_size=self.g_mask_dim)

        self.layout_to_image = define_G(self.num_objs + rep_size, 3, ngf, n_downsample_global, n_blocks_global,
                                        'instance')
        # hooks that are not part of the reference surface
        self.noise_override = None          # (1, mask_noise_dim) row used instead of torch.randn (parity tests), or (N, mask_noise_dim): one row per image
        self.layout_objects_hint = 0        # objects/image the layout kernel provisions LDS for (0 = default 12)
        self.objs_host = None               # optional host copies of ``objs`` / ``obj_to_img`` (lists): skip the one
        self.obj_to_img_host = None         # D2H copy per forward that VectorPool and the sparse first conv need
        self.lazy_layouts = False           # defer the dense layout kernels until a dense read (see forward)
        self.rep_size = rep_size
        # ---- sampling (scene_generation_amd/sample.py) ----
        # the appearance banks scripts/gui/model.py:47-55 hangs on the model: {class id: array [rows, rep_size]} with up to 100
        # rows per class (``features``) and one row per class (``features_one``); read by encode_scene_graphs
        self.features = None
        self.features_one = None
        # test-mode forward on the FACTORED layout (one value plane per object + the winner plane,
        # ops.masks_to_layout_test_planes) instead of the dense (N, num_objs + rep_size, H, W) tensor.  Off: forward is unchanged.
        # On, the returned pred_layout is a DEFERRED tensor -- uninitialised memory until ops.ensure_dense(pred_layout), exactly
        # like the layouts of ``lazy_layouts`` -- and carries the hint 'test_planes' = (winner, value) for ops.layout_rgb.
        self.factored_test_layout = False

    def forward(self, gt_imgs, objs, triples, obj_to_img, boxes_gt=None, masks_gt=None, attributes=None,
                test_mode=False, use_gt_box=False, features=None):
        ops.clear_hints()                        # layout hints of the previous iteration (and the tensors they pin)
        O = objs.size(0)
        objs_h, o2i_h = self.objs_host, self.obj_to_img_host
        if objs_h is None or o2i_h is None:      # one sync (the reference's pool does objs.tolist(), utils.py:104)
            objs_h, o2i_h = torch.stack((objs, obj_to_img)).tolist()
        N = gt_imgs.size(0) if gt_imgs is not None else max(o2i_h) + 1
        lazy = self.lazy_layouts and ops.FACTORED_LAYOUT
        # The OBJECT FRONT -- embeddings, graph convolutions, box_net, mask_net -- and the IMAGE PATH of the training branch --
        # crops, AppearanceEncoder, the layouts built from the ground-truth boxes and masks, the generator (model.py:98-124) --
        # share no tensor: boxes_pred / masks_pred feed losses and the (deferred) pred_layout only.  The front is ~100 launches of
        # a few microseconds forward and ~250 backward; on a side stream (streams.fork, group 'front') they run beside the
        # generator's GEMMs, forward here and backward wherever autograd runs the nodes recorded on that stream.  Only when the
        # dense pred_layout is deferred (Trainer.step) and no inference-time features are given; results are bit-identical.
        side = lazy and not test_mode and features is None
        with streams.fork(objs.device, 'front', enabled=side) as fk:
            with fk.branch(1, reads=(objs, triples, attributes)):
                obj_vecs, pred_vecs = self.scene_graph_to_vectors(objs, triples, attributes)
                box_vecs, mask_vecs = obj_vecs, self._mask_vecs(obj_vecs, O, obj_to_img)
                boxes_pred = self.box_net(box_vecs)
                mask_scores = self.mask_net(mask_vecs.view(O, -1, 1, 1))
                masks_pred = ops.activation(mask_scores.squeeze(1), ops.ACT_SIGMOID)
                fk.produced((boxes_pred, masks_pred, mask_vecs))
            scene_layout_vecs, wrong_layout_vecs = self._appearance_vecs(gt_imgs, boxes_gt, obj_to_img, objs, mask_vecs, features,
                                                                         objs_host=objs_h)
            return self._layouts_and_image(gt_imgs, objs, obj_to_img, boxes_gt, masks_gt, boxes_pred, masks_pred,
                                           scene_layout_vecs, wrong_layout_vecs, objs_h, o2i_h, N, lazy, test_mode, use_gt_box)

    def _layouts_and_image(self, gt_imgs, objs, obj_to_img, boxes_gt, masks_gt, boxes_pred, masks_pred, scene_layout_vecs,
                           wrong_layout_vecs, objs_h, o2i_h, N, lazy, test_mode, use_gt_box):
        H, W = self.image_size
        kw = dict(num_images=N, validate=False, max_per_image=self.layout_objects_hint)
        if test_mode:                                      # model.py:111-117
            boxes = boxes_gt if use_gt_box else boxes_pred
            masks = masks_gt if masks_gt is not None else masks_pred
            if self.factored_test_layout and ops.FACTORED_LAYOUT:
                return self._factored_test_image(objs, obj_to_img, boxes, masks, boxes_pred, masks_pred, scene_layout_vecs,
                                                 o2i_h, N)
            pred_layout = masks_to_layout(scene_layout_vecs, boxes, masks, obj_to_img, H, W, test_mode=True,
                                          num_images=N, validate=False)
            ops.set_hints(pred_layout, sparse=tuple(
                to_device_async(torch.from_numpy(a), pred_layout.device)
                for a in active_layout_channels(objs_h, o2i_h, N, self.num_objs, self.rep_size)))
            return self.layout_to_image(pred_layout), boxes_pred, masks_pred, None, pred_layout, None
        seg = ops.segment_offsets(obj_to_img, N)
        if lazy:
            # nothing on the training step reads the dense layouts (the convs over them run on the factored form): their
            # kernels are deferred until a dense read (ops.ensure_dense; Trainer.step does it for the outputs it returns)
            def layout_of(vecs, masks):
                return ops.masks_to_layout_deferred(vecs, boxes_gt, masks, seg, N, H, W, False, self.layout_objects_hint,
                                                    differentiable=vecs.requires_grad)
        else:
            def layout_of(vecs, masks):
                return masks_to_layout(vecs, boxes_gt, masks, obj_to_img, H, W, test_mode=False,
                                       grad_from_channel=self.num_objs, **kw)
        gt_layout = layout_of(scene_layout_vecs, masks_gt)
        # pred_layout feeds no loss (train.py:203,219); it stays differentiable w.r.t. masks_pred like the reference's
        pred_layout = layout_of(scene_layout_vecs, masks_pred)
        wrong_layout = layout_of(wrong_layout_vecs, masks_gt)
        dev = gt_layout.device
        if not ops.FACTORED_LAYOUT:
            # per image only the one-hot planes of its own classes + the representation block are non-zero: the
            # generator's first conv (204 -> 64 channels, 7x7, full resolution) skips the rest
            sparse = tuple(to_device_async(torch.from_numpy(a), dev)
                           for a in active_layout_channels(objs_h, o2i_h, N, self.num_objs, self.rep_size))
            # same lists + the 3 image channels the image discriminator concatenates behind the layout
            sparse_img = tuple(to_device_async(torch.from_numpy(a), dev)
                               for a in active_layout_channels(objs_h, o2i_h, N, self.num_objs, self.rep_size, extra=3))
            for lay in (gt_layout, pred_layout, wrong_layout):
                ops.set_hints(lay, sparse=sparse, sparse_cat={3: sparse_img})
        if ops.FACTORED_LAYOUT:
            # factored form of the two layouts that feed convolutions: planes S_o + per-object vectors (ops.FactoredLayout)
            counts = [0] * N
            plane = []
            for i in o2i_h:
                plane.append(counts[i])
                counts[i] += 1
            pidx = to_device_async(torch.tensor(plane, dtype=torch.int64), dev)
            Z = ops.layout_planes(boxes_gt, masks_gt, seg, pidx, N, max(counts), H, W)
            f_gt = ops.FactoredLayout(Z, objs, scene_layout_vecs[:, self.num_objs:], self.num_objs, obj_to_img, pidx, counts, seg)
            f_wrong = ops.FactoredLayout(Z, objs, wrong_layout_vecs[:, self.num_objs:].detach(), self.num_objs, obj_to_img,
                                         pidx, counts, seg)
            f_wrong._lists = f_gt._lists          # same objects: share the list cache
            # 'wrong_twin': the image discriminator sees (layout, real image) and (wrong layout, real image) -- same planes, same
            # objects, other appearance vectors -- and can run the two passes as ONE batch (Trainer.train_generator)
            ops.set_hints(gt_layout, factored=f_gt, wrong_twin=f_wrong)
            ops.set_hints(wrong_layout, factored=f_wrong)
        imgs_pred = self.layout_to_image(gt_layout)
        return imgs_pred, boxes_pred, masks_pred, gt_layout, pred_layout, wrong_layout

    def _factored_test_image(self, objs, obj_to_img, boxes, masks, boxes_pred, masks_pred, layout_vecs, o2i_h, N):
        """The test-mode branch of forward without the dense layout.  Every pixel belongs to at most one object (the first, in
        ascending mass, whose sampled mask exceeds 0.5: layout.py:157-169), so layout = vecs[winner(p)] * value(p) = sum_o vecs[o]
        (x) Z_o with Z_o = value where o wins and 0 elsewhere: the planes x per-object-filters form the training stem already runs
        on (ops.FactoredLayout; vecs = [one_hot | repr] and 'sum' pooling here as there)."""
        H, W = self.image_size
        dev = layout_vecs.device
        seg = ops.segment_offsets(obj_to_img, N)
        counts, plane = [0] * N, []
        for i in o2i_h:
            plane.append(counts[i])
            counts[i] += 1
        pidx = to_device_async(torch.tensor(plane, dtype=torch.int64), dev)
        Z, winner, value = ops.masks_to_layout_test_planes(layout_vecs, boxes, masks, seg, pidx, N, max(counts), H, W, False)
        pred_layout = ops.masks_to_layout_test_deferred(layout_vecs, boxes, masks, seg, N, H, W, False)
        f = ops.FactoredLayout(Z, objs, layout_vecs[:, self.num_objs:].detach(), self.num_objs, obj_to_img, pidx, counts, seg)
        ops.set_hints(pred_layout, factored=f, test_planes=(winner, value))
        return self.layout_to_image(pred_layout), boxes_pred, masks_pred, None, pred_layout, None

    def encode_scene_graphs(self, scene_graphs, rand=False, *, fix_feature_classes=False):
        """model.py:174-250: scene graphs written by a person ({'objects': [names], 'relationships': [[s, name, o]], 'attributes':
        {'size': [...], 'location': [...]}, 'features': [bank row per object], 'image_id': bank row of the image}) ->
        (objs, triples, obj_to_img, attributes, features) on the model's device.  What the reference does is reproduced, the
        unexpected included ("sampling"):
          * it APPENDS to the caller's dicts: '__image__' to objects, image_id to features, one __in_image__ triple per object
          * the attribute block is 35 columns wide whatever the vocabulary says; the __image__ row gets columns 9 and 22
          * feature number -1 takes row 0 of ``features_one``; any other is clamped to row 99 of ``features``
          * the bank is looked up by zipping the CUMULATIVE object list with the graph's feature numbers, so the objects of the
            second and later graphs are served from the classes at the START of the list.  ``fix_feature_classes=True`` (not in
            the reference) looks the graph's own classes up instead.
        ``rand`` is accepted and ignored, as in the reference."""
        import numpy as np
        if isinstance(scene_graphs, dict):
            scene_graphs = [scene_graphs]
        device = next(self.parameters()).device
        vocab = self.vocab
        objs, triples, obj_to_img, all_attributes, feats = [], [], [], [], []
        obj_offset = 0
        for i, sg in enumerate(scene_graphs):
            attributes = np.zeros((len(sg['objects']) + 1, 25 + 10), dtype=np.float32)
            sg['objects'].append('__image__')
            sg['features'].append(sg['image_id'])
            image_idx = len(sg['objects']) - 1
            for j in range(image_idx):
                sg['relationships'].append([j, '__in_image__', image_idx])
            for obj in sg['objects']:
                if obj not in vocab['object_name_to_idx']:       # (a KeyError in the reference, whose None check never fires)
                    raise ValueError('Object "%s" not in vocab' % obj)
                obj_idx = vocab['object_to_idx'][str(vocab['object_name_to_idx'][obj])]
                if obj_idx is None:
                    raise ValueError('Object "%s" not in vocab' % obj)
                objs.append(obj_idx)
                obj_to_img.append(i)
            if self.features is not None:
                classes = objs[obj_offset:] if fix_feature_classes else objs
                for cls, feat_num in zip(classes, sg['features']):
                    if feat_num == -1:
                        feat = self.features_one[cls][0]
                    else:
                        feat = self.features[cls][min(feat_num, 99), :]
                    feats.append(np.asarray(feat))
            for s, p, o in sg['relationships']:
                pred_idx = vocab['pred_name_to_idx'].get(p, None)
                if pred_idx is None:
                    raise ValueError('Relationship "%s" not in vocab' % p)
                triples.append([s + obj_offset, pred_idx, o + obj_offset])
            for k, size_attr in enumerate(sg['attributes']['size']):
                attributes[k, size_attr] = 1
            attributes[-1, 9] = 1                                # the image's size ...
            for k, location_attr in enumerate(sg['attributes']['location']):
                attributes[k, location_attr + 10] = 1
            attributes[-1, 12 + 10] = 1                          # ... and location
            obj_offset += len(sg['objects'])
            all_attributes.append(attributes)
        # one host-to-device copy per output (the reference: one per feature row)
        features = []
        if feats:
            bank = to_device_async(torch.from_numpy(np.stack(feats).astype(np.float32)), device)
            features = list(bank.unbind(0))
        objs = to_device_async(torch.tensor(objs, dtype=torch.int64), device)
        triples = to_device_async(torch.tensor(triples, dtype=torch.int64), device)
        obj_to_img = to_device_async(torch.tensor(obj_to_img, dtype=torch.int64), device)
        attributes = to_device_async(torch.from_numpy(np.concatenate(all_attributes)), device)
        return objs, triples, obj_to_img, attributes, features

    def forward_json(self, scene_graphs):
        """model.py:252-256: encode_scene_graphs + forward(test_mode=True, predicted boxes and masks) -> (forward's tuple, objs)"""
        objs, triples, obj_to_img, attributes, features = self.encode_scene_graphs(scene_graphs)
        return self.forward(None, objs, triples, obj_to_img, attributes=attributes, test_mode=True, use_gt_box=False,
                            features=features), objs

    def scene_graph_to_vectors(self, objs, triples, attributes):
        s, p, o = triples[:, 0], triples[:, 1], triples[:, 2]
        edges = torch.stack([s, o], dim=1)                   # index plumbing (T x 2 int64)
        obj_vecs = self.obj_embeddings(objs)
        pred_vecs = self.pred_embeddings(p.contiguous())
        if self.use_attributes:
            obj_vecs = ops.concat_cols(obj_vecs, attributes)
        # the destination-major CSR of the triples (segmented pool, gather adjoint): built once for all graph-conv layers
        csr = ops.build_csr(edges, objs.numel()) if objs.is_cuda else None
        if isinstance(self.gconv, Linear):
            obj_vecs = self.gconv(obj_vecs)
        else:
            obj_vecs, pred_vecs = self.gconv(obj_vecs, pred_vecs, edges, csr=csr)
        if self.gconv_net is not None:
            obj_vecs, pred_vecs = self.gconv_net(obj_vecs, pred_vecs, edges, csr=csr)
        return obj_vecs, pred_vecs

    def create_components_vecs(self, imgs, boxes, obj_to_img, objs, obj_vecs, features, objs_host=None):
        """model.py:146-172 -- the reference's method, kept whole for callers of the reference surface; forward() runs its two
        halves separately (the first belongs to the object front, the second to the image path)."""
        mask_vecs = self._mask_vecs(obj_vecs, objs.size(0), obj_to_img)
        layout_vecs, wrong_layout_vecs = self._appearance_vecs(imgs, boxes, obj_to_img, objs, mask_vecs, features,
                                                               objs_host=objs_host)
        return obj_vecs, mask_vecs, layout_vecs, wrong_layout_vecs

    def _mask_vecs(self, obj_vecs, O, obj_to_img=None):
        if self.noise_override is not None and self.noise_override.dim() == 2 and self.noise_override.size(0) != 1:
            # one row per IMAGE (qmc.QuasiRandomInputs): object o takes the row of its image, a device gather
            if obj_to_img is None:
                raise ValueError('a noise_override of %d rows is one row per image: _mask_vecs needs obj_to_img'
                                 % self.noise_override.size(0))
            noise = self.noise_override.to(obj_vecs.device, obj_vecs.dtype).view(-1, self.mask_noise_dim)
            return ops.concat_cols(obj_vecs, ops.embedding(noise.contiguous(), obj_to_img))     # (sg_embedding_fwd: a row gather)
        if self.noise_override is not None:
            noise = self.noise_override.to(obj_vecs.device, obj_vecs.dtype).view(1, self.mask_noise_dim)
        else:                                                # ONE noise row per batch (model.py:149-151)
            noise = torch.randn((1, self.mask_noise_dim), dtype=obj_vecs.dtype, device=obj_vecs.device)
        return ops.concat_cols(obj_vecs, noise.expand(O, self.mask_noise_dim))

    def _appearance_vecs(self, imgs, boxes, obj_to_img, objs, mask_vecs, features, objs_host=None):
        if features is None:
            crops = crop_bbox_batch(imgs, boxes, obj_to_img, self.object_size)
            obj_repr = self.repr_net(self.image_encoder(crops))
        elif torch.is_tensor(features):                      # every object's appearance row, already on the device (qmc.DeviceBank)
            if features.dim() != 2 or tuple(features.shape) != (objs.size(0), self.rep_size):
                raise ValueError('features as a tensor must be [%d, %d] (one row of rep_size per object), got %s'
                                 % (objs.size(0), self.rep_size, tuple(features.shape)))
            if not features.is_floating_point() or features.device != mask_vecs.device:
                raise ValueError('features as a tensor must be a float tensor on %s, got %s on %s'
                                 % (mask_vecs.device, features.dtype, features.device))
            obj_repr = features.to(mask_vecs.dtype)          # replaces repr_net's output whole: nothing to compute, nothing to index
        else:                                                # only at inference time (model.py:158-163)
            obj_repr = self.repr_net(mask_vecs)
            rows = [i for i, f in enumerate(features) if f is not None]
            if rows:
                obj_repr = obj_repr.clone()
                obj_repr[torch.tensor(rows, device=obj_repr.device)] = torch.stack(
                    [torch.as_tensor(features[i], dtype=obj_repr.dtype).to(obj_repr.device).view(-1) for i in rows])

        one_hot_obj = ops.one_hot(objs, self.num_objs)
        layout_vecs = ops.concat_cols(one_hot_obj, obj_repr)

        wrong_objs_rep = self.fake_pool.query(objs, obj_repr, objs_host=objs_host if objs_host is not None else self.objs_host)
        wrong_layout_vecs = ops.concat_cols(one_hot_obj, wrong_objs_rep)
        return layout_vecs, wrong_layout_vecs
