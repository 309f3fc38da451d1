"""Pictures and captions to the denoiser's inputs, one batch ahead of the training step: the part of reference train_scripts/train.py:140-168 that runs
between the DataLoader and `training_losses` when a config sets load_vae_feat = False (and load_t5_feat = False).

PictureBatches is an iterator of (x0, y, mask, data_info) - x0 fp32 (B, 4, h, w) already multiplied by the scale factor, y fp32 (B, 1, L, 4096) on the device,
mask int64 (B, L) on the host, data_info = {img_hw (B, 2), aspect_ratio (B, 1)} - the tuple train.py's feature_batches yields.  Per batch:

    index order      torch.randperm(len(dataset), generator) [rank::world] -> AspectRatioBatchSampler, the path of feature_batches (one bucket per batch),
                     with the permutation drawn from the seed alone so that the ranks' slices are disjoint; a fixed-resolution dataset (ratios None) is
                     cut into consecutive batches of that order
    decode           dataset.decode(idx) on a thread pool of min(num_workers, 8) threads (never sized from the machine's CPU count), each thread
                     uploading its picture's bytes on ONE side stream: to_device_u8(stream=...)
    transform        ImagePreprocessor(dataset.form, dataset.filter) into the slots of one fp32 (B, 3, H, W) batch - kept as `self.pictures`
    latents          vae.encode_latents(pictures, scale, sample, noise): the encoder's launches and pxa_vae_posterior
    captions         text: captions.submit(texts) when the batch is begun, captions.collect() when it is finished (CaptionEncoder; under the f16 build the
                     round trip to its worker); caption files: dataset.caption_features, read by the decode threads

The batch after the one being handed out is BEGUN (decodes queued, captions submitted) before the current one is finished, so decoding and the caption
round trip run while the caller's previous step occupies the GPU.

Determinism.  Every random draw - the permutation, the caption kind per item, the index replacing an undecodable picture, the posterior's noise - is made
on the iterating thread, in item order, from generators seeded with seed (the permutation) and seed + rank (the rest); the threads only decode, and their
results are taken in item order.  Two iterators with one seed therefore yield the same pictures, captions, masks, data_info and noise, bit for bit, whatever
the thread timing; x0 is as repeatable as two encodes of one tensor are (the GroupNorm statistics of the encoder are accumulated with atomics: DESIGN.md
section 4g)."""
import time
from concurrent.futures import ThreadPoolExecutor

import torch

from .images import ImagePreprocessor, to_device_u8
from .pictures import RETRIES
from .sampler import AspectRatioBatchSampler

MAX_THREADS = 8


class _Batch:
    """One batch between `begin` and `finish`: item indices, caption draws (real prompt?, text, feature file), decode futures, the text path's host mask."""

    def __init__(self, idx, caps, futures, mask):
        self.idx, self.caps, self.futures, self.mask, self.loaded = idx, caps, futures, mask, None


class PictureBatches:
    def __init__(self, dataset, batch_size, ratios, vae, captions, seed, rank=0, world=1, device="cuda", num_workers=4, valid_num=0, scale=None,
                 sample_posterior=True, profile=False):
        if captions is None and not dataset.load_t5_feat:
            raise ValueError("PictureBatches needs a CaptionEncoder, or a dataset built with load_t5_feat=True (caption feature files)")
        self.dataset, self.batch_size, self.ratios, self.vae, self.captions = dataset, int(batch_size), ratios, vae, captions
        self.seed, self.rank, self.world, self.valid_num = int(seed), int(rank), int(world), valid_num
        self.device = torch.device(device)
        self.scale, self.sample_posterior = scale, bool(sample_posterior)
        self.threads = max(1, min(int(num_workers), MAX_THREADS))
        self.pictures = self.noise = self.indices = self.texts = None      # of the batch handed out last
        self.profile, self.timing = bool(profile), {}                      # profile: synchronise between the phases and keep their seconds (bench tool)

    # ---- index order
    def index_batches(self):
        """The item indices of batch after batch, epoch after epoch.  The permutation of an epoch is drawn from the seed alone, so that the ranks cut disjoint
        slices [rank::world] out of ONE order (every other draw is the rank's own: seed + rank)."""
        ds, B = self.dataset, self.batch_size
        g = torch.Generator().manual_seed(self.seed)
        while True:
            order = torch.randperm(len(ds), generator=g).tolist()[self.rank::self.world]
            if self.ratios is None:
                full = [order[i:i + B] for i in range(0, len(order) - B + 1, B)]
            else:
                full = AspectRatioBatchSampler(order, ds, B, self.ratios, drop_last=True, valid_num=self.valid_num,
                                               ratio_nums={str(k): v for k, v in ds.ratio_nums.items()})
            n = 0
            for idx in full:
                n += 1
                yield list(idx)
            if n == 0:
                raise RuntimeError(f"no full batch of {B} among the {len(order)} items of rank {self.rank}: nothing to train on")

    # ---- one picture, on a pool thread: decode, upload on the side stream (and read the caption file, when captions are files)
    def _load(self, idx, npz, side):
        pic = to_device_u8(self.dataset.decode(idx), self.device, stream=side)
        return pic, (self.dataset.caption_features(npz) if self.captions is None else None)

    def _begin(self, pool, side, idx, g):
        caps = [self.dataset.caption(i, g) for i in idx]                    # drawn in item order, on this thread
        futures = [pool.submit(self._load, i, c[2], side) for i, c in zip(idx, caps)]
        mask = self.captions.submit([c[1] for c in caps]) if self.captions is not None else None
        return _Batch(idx, caps, futures, mask)

    def _settle(self, b, side, g):
        """Wait for the batch's decodes; replace what could not be decoded the way the dataset's __getitem__ does (a new index and a new caption draw per
        attempt, 20 attempts in all), on this thread and in item order."""
        ds, replaced = self.dataset, False
        b.loaded = []
        for slot, f in enumerate(b.futures):
            try:
                b.loaded.append(f.result())
                continue
            except Exception as e:      # noqa: BLE001  (the reference catches everything, prints, and tries another item)
                err = e
            for _ in range(RETRIES - 1):
                print(f"Error details {ds.img_samples[b.idx[slot]]}: {err}")
                b.idx[slot] = ds.replacement(b.idx[slot], g)
                b.caps[slot] = ds.caption(b.idx[slot], g)
                replaced = True
                try:
                    b.loaded.append(self._load(b.idx[slot], b.caps[slot][2], side))
                    break
                except Exception as e:      # noqa: BLE001
                    err = e
            else:
                raise RuntimeError("Too many bad data.")
        if replaced and self.captions is not None:                         # the texts submitted when the batch was begun are stale: encode again
            self.captions.collect()
            b.mask = self.captions.submit([c[1] for c in b.caps])
        b.futures = None

    def _finish(self, b, gpu_gen):
        ds, dev = self.dataset, self.device
        marks = [time.perf_counter()]

        def mark():
            if self.profile:
                torch.cuda.synchronize(dev)
            marks.append(time.perf_counter())
        H, W = ds.output_hw(b.idx[0])
        pictures = torch.empty(len(b.idx), 3, H, W, dtype=torch.float32, device=dev)
        for slot, (pic, _) in enumerate(b.loaded):
            self._pre(pic, ds.target(b.idx[slot]), out=pictures, slot=slot)
        mark()
        lc, f = self.vae.config.latent_channels, 1 << (len(self.vae.config.block_out_channels) - 1)
        noise = torch.randn((len(b.idx), lc, H // f, W // f), generator=gpu_gen, device=dev, dtype=torch.float32) if self.sample_posterior else None
        x0 = self.vae.encode_latents(pictures, scale=self.scale, sample=self.sample_posterior, noise=noise)
        mark()
        if self.captions is not None:
            y, mask = self.captions.collect(), b.mask
        else:
            y = torch.stack([c[0].float() for _, c in b.loaded]).to(dev)                            # (B, 1, L, 4096)
            mask = torch.cat([c[1].reshape(1, -1) for _, c in b.loaded]).long()                     # host mask: no device sync for the caption lengths
        mark()
        infos = [ds.data_info(i) for i in b.idx]
        info = {"img_hw": torch.stack([d["img_hw"] for d in infos]), "aspect_ratio": torch.tensor([[float(d["aspect_ratio"])] for d in infos])}
        self.pictures, self.noise, self.indices, self.texts = pictures, noise, list(b.idx), [c[1] for c in b.caps]
        self.timing.update(transform=marks[1] - marks[0], vae_encode=marks[2] - marks[1], captions=marks[3] - marks[2])
        return x0, y, mask, info

    def __iter__(self):
        ds = self.dataset
        g = torch.Generator().manual_seed(self.seed + self.rank)
        gpu_gen = torch.Generator(device=self.device).manual_seed(self.seed + self.rank)
        self._pre = ImagePreprocessor(ds.form, ds.filter, self.device)
        side = torch.cuda.Stream(device=self.device)
        batches = self.index_batches()
        pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="pxa-decode")
        try:
            nxt = self._begin(pool, side, next(batches), g)
            while True:
                cur = nxt
                t0 = time.perf_counter()
                self._settle(cur, side, g)                                 # its replacements draw before the next batch's caption kinds: a fixed order
                self.timing = {"decode_wait": time.perf_counter() - t0}
                nxt = self._begin(pool, side, next(batches), g)
                yield self._finish(cur, gpu_gen)
        finally:
            pool.shutdown(wait=True, cancel_futures=True)
            try:
                while self.captions is not None and self.captions.outstanding:     # the batch begun ahead: take its features off the encoder's queue
                    self.captions.collect()
            except RuntimeError:                                               # a failed worker has raised where it failed, and stays failed
                pass
