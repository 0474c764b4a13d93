"""Benchmark of the Pillow-exact device resize (scene_generation_amd/imageprep.py, csrc/imageprep.hip) on cuda:0.

(a) ``resize``: ``--batch`` images of 480 x 640 to 128 x 128 and to 299 x 299, both filters.  Per launch of ``sg_pil_resize``
    (coefficients, horizontal, vertical: issued alone through the ``phases`` bits over a table uploaded once) and for the three
    together: time, the bytes the launch moves (computed from the shapes below) and their rate as a share of the 6.29 TB/s copy rate
    measured on this part.  ``resize_call`` is ``ops.pil_resize`` as a user issues it: the plan, the table upload and the launches.
(b) ``host_pillow``: the same images through ``Image.resize`` and ``inception.read_image``'s expression, one thread.
(c) ``fid_real_feed``: the real side of ``python -m scene_generation_amd.fid`` (``fid._feed_dir`` into ``add_real``, random weights)
    over a generated directory of ``--files`` PNGs in 8 sizes interleaved in sorted order: images per second without the flag (the
    files at their stored sizes: a new chunk at every size change) and with ``--image_size 128,128``, back to back, and the parts of
    the flagged run taken alone -- decoding (the feeder's thread pool, nothing else), packing + upload + resize (decoded arrays in
    memory), the Inception forward of as many 128 x 128 batches -- to say which one bounds it.

The method is tools/bench_fid.py's for the device figures: warmed up, the median of ``--blocks`` blocks of at least ``--seconds`` each
by the host clock around a device synchronise, with the spread and the same launches between two device events.  Nothing is
asserted.  One JSON line per figure, appended to profiles/imageprep_bench.jsonl (or --out)."""
import argparse
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from scene_generation_amd import fid as FID  # noqa: E402
from scene_generation_amd import imageprep as IP  # noqa: E402
from scene_generation_amd import ops  # noqa: E402
from tools.benchkit import emit, measure, require_device  # noqa: E402

DEV = 'cuda:0'
COPY_RATE = 6.29e12                 # bytes / s: the copy rate measured on the MI355X
SIZES8 = [(480, 640), (427, 640), (640, 480), (500, 375), (375, 500), (640, 427), (480, 360), (333, 500)]


_BASE = {}


def picture(rs, h, w):
    """a smooth picture with some noise: compresses and decodes like a photograph rather than like noise.  One smooth base per size
    (the transcendental part), shifted and re-noised per call."""
    if (h, w) not in _BASE:
        y, x = np.mgrid[0:h, 0:w].astype(np.float32)
        base = np.stack([np.sin(x / rs.uniform(20, 80) + rs.uniform(0, 6)) * np.cos(y / rs.uniform(20, 80)) for _ in range(3)], 2)
        _BASE[(h, w)] = np.clip(127.5 + 100 * base, 8, 247).astype(np.uint8)
    shifted = np.roll(_BASE[(h, w)], (int(rs.randint(h)), int(rs.randint(w))), axis=(0, 1))
    return shifted + rs.randint(0, 9, size=(h, w, 3)).astype(np.uint8) - 4


def launch_bytes(n, H, W, OH, OW, ksize_h, ksize_v, u8, f32):
    coef = n * 4.0 * ((ksize_h + 2) * OW + (ksize_v + 2) * OH)
    inter = n * 3.0 * H * OW
    return {'coef': coef, 'horizontal': n * 3.0 * H * W + inter, 'vertical': inter + n * 3.0 * OH * OW * ((1 if u8 else 0) + (4 if f32 else 0))}


def bench_resize(args, base):
    rs = np.random.RandomState(0)
    H, W = 480, 640
    arrays = [picture(rs, H, W) for _ in range(args.batch)]
    packed, desc = IP.pack_images(arrays)
    dev = packed.to(DEV)
    L = ops._L()
    for size in ((128, 128), (299, 299)):
        for filt in ('bilinear', 'bicubic'):
            OH, OW = size
            n = len(arrays)
            host, totals = np.empty((n + 1, ops.imageprep._TABLE_COLS), np.int64), np.empty(4, np.int64)
            assert L.sg_pil_resize_plan(desc.ctypes.data, n, dev.numel(), OH, OW, ops.PIL_FILTERS[filt], host.ctypes.data, totals.ctypes.data) == 0
            coef_ints, inter_bytes, hblocks, nbytes = (int(v) for v in totals)
            table = torch.from_numpy(host).to(DEV)
            ws = ops.workspace(nbytes, torch.device(DEV))
            y = torch.empty(n, 3, OH, OW, device=DEV)
            lut = ops.imageprep._lut(torch.device(DEV))

            def launch(phases):
                ops._call('sg_pil_resize', dev.data_ptr(), dev.numel(), table.data_ptr(), n, OH, OW, ops.PIL_FILTERS[filt], coef_ints,
                          inter_bytes, hblocks, lut.data_ptr(), None, y.data_ptr(), ws.data_ptr(), ws.numel(), phases, ops._stream())

            by = launch_bytes(n, H, W, OH, OW, int(host[0, 5]), int(host[0, 6]), False, True)
            by['all'] = sum(by.values())
            launch(ops.PIL_ALL)
            for name, phases in (('coef', ops.PIL_COEF), ('horizontal', ops.PIL_HORIZONTAL), ('vertical', ops.PIL_VERTICAL), ('all', ops.PIL_ALL)):
                r = measure(lambda: launch(phases), args.seconds, args.blocks, clocks=True)
                rate = by[name] / (r['device_events_ms'] * 1e-3)
                emit(args.out, dict(base, figure='resize_launch', launch=name, batch=n, source=[H, W], target=list(size), filter=filt,
                                    bytes=by[name], bytes_per_s=rate, share_of_copy_rate=rate / COPY_RATE,
                                    hbm_floor_us=by[name] / COPY_RATE * 1e6, **r))
            r = measure(lambda: ops.pil_resize(dev, desc, size, filt, out=y), args.seconds, args.blocks, clocks=True)
            emit(args.out, dict(base, figure='resize_call', batch=n, source=[H, W], target=list(size), filter=filt, bytes=by['all'], **r))
            # (b) the host alternative, one thread
            from PIL import Image
            res = {'bilinear': Image.BILINEAR, 'bicubic': Image.BICUBIC}[filt]
            threads = torch.get_num_threads()
            torch.set_num_threads(1)
            try:
                times = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    out = [(torch.from_numpy(np.asarray(Image.fromarray(a).resize((OW, OH), res), dtype=np.float32)).permute(2, 0, 1)
                            / 255.0 - 0.5) / 0.5 for a in arrays]
                    times.append((time.perf_counter() - t0) * 1e3)
            finally:
                torch.set_num_threads(threads)
            same = bool(torch.equal(torch.stack(out), y.cpu()))
            emit(args.out, dict(base, figure='host_pillow', batch=n, source=[H, W], target=list(size), filter=filt, ms=sorted(times)[1],
                                runs_ms=times, threads=1, device_output_bit_equal=same))


def bench_feed(args, base):
    from PIL import Image
    root = tempfile.mkdtemp(prefix='imageprep_bench_')
    try:
        rs = np.random.RandomState(1)
        for i in range(args.files):
            h, w = SIZES8[i % len(SIZES8)]
            Image.fromarray(picture(rs, h, w)).save(os.path.join(root, '%04d.png' % i), compress_level=1)
        fid = FID.FrechetInceptionDistance(weights=None, batch_size=args.batch, device=DEV)
        chunks = []

        def feed(imgs):
            chunks.append(int(imgs.size(0)))
            fid.add_real(imgs)

        def run(**kw):
            fid.clean_real()
            del chunks[:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            FID._feed_dir(feed, root, args.batch, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        flag = dict(image_size=(128, 128), resize_filter='bilinear', device=torch.device(DEV))
        run()
        run(**flag)                                     # both paths warmed up (code objects, the page-locked slots, the file cache)
        rounds = []
        for _ in range(args.feed_rounds):               # back to back, alternating
            t_plain = run()
            n_plain = len(chunks)
            t_flag = run(**flag)
            rounds.append({'plain_s': t_plain, 'plain_chunks': n_plain, 'flag_s': t_flag, 'flag_chunks': len(chunks)})
        med = lambda key: sorted(r[key] for r in rounds)[len(rounds) // 2]
        # the parts of the flagged run, each alone
        feeder = IP.ImageDirFeeder(root, args.batch, (128, 128), 'bilinear', DEV)
        from concurrent.futures import ThreadPoolExecutor
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=feeder.workers) as pool:
            arrays = list(pool.map(IP.decode, feeder.paths))
        t_decode = time.perf_counter() - t0
        slots = [dict(), dict()]
        groups = [arrays[a:a + args.batch] for a in range(0, len(arrays), args.batch)]

        def resize_all():
            out = None
            for k, g in enumerate(groups):
                p, t = feeder._upload(slots[k % 2], g)
                out = ops.pil_resize(p, t, (128, 128), 'bilinear')
            return out
        resize_all()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch = resize_all()
        torch.cuda.synchronize()
        t_resize = time.perf_counter() - t0
        full = batch if batch.size(0) == args.batch else torch.zeros(args.batch, 3, 128, 128, device=DEV)
        fid.clean_real()
        fid.add_real(full)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in groups:
            fid.add_real(full)
        torch.cuda.synchronize()
        t_net = time.perf_counter() - t0
        parts = {'decode_s': t_decode, 'pack_upload_resize_s': t_resize, 'inception_s': t_net}
        emit(args.out, dict(base, figure='fid_real_feed', files=args.files, sizes=SIZES8, batch=args.batch, rounds=rounds,
                            decode_workers=feeder.workers, plain_images_per_s=args.files / med('plain_s'),
                            flag_images_per_s=args.files / med('flag_s'), plain_chunks=rounds[0]['plain_chunks'],
                            flag_chunks=rounds[0]['flag_chunks'], flag_parts=parts, flag_bound_by=max(parts, key=parts.get)))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=32)
    p.add_argument('--files', type=int, default=256)
    p.add_argument('--feed_rounds', type=int, default=3)
    p.add_argument('--seconds', type=float, default=0.3)
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--skip', nargs='*', default=[], choices=['resize', 'feed'])
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'imageprep_bench.jsonl'))
    args = p.parse_args(argv)
    require_device()
    import PIL
    base = {'device': torch.cuda.get_device_name(0), 'host_threads': torch.get_num_threads(), 'pillow': PIL.__version__}
    if 'resize' not in args.skip:
        bench_resize(args, base)
    if 'feed' not in args.skip:
        bench_feed(args, base)


if __name__ == '__main__':
    main()
