"""`casapose.data_handler.image_only_dataset.ImageOnlyDataset` of the reference (image_only_dataset.py:8-106): plain camera frames, no
annotations, as network input for the inference-only driver (util_scripts/test_minimal.py).

Discovery: every LEAF folder under `root` (a folder without subfolders; subfolders are visited in sorted order) contributes its sorted
`*[0-9].png` files, or its sorted `*[0-9].jpg` files when it has no such PNG; `NNNNNN.seg.png` masks therefore never match.

Decoding happens on the host with PIL into uint8 arrays with the channel counts of TF's `decode_image`: L -> 1, RGB -> 3, RGBA -> 4, a palette
image -> RGB (RGBA when it has a transparency entry), a bilevel image -> L.  Two-channel (LA) and 16-bit images are refused by name: the reference
cannot turn them into a three-channel 8-bit input either.  JPEG frames decode through libjpeg in PIL; TF's decoder may round a few pixels
differently, PNG frames are the same bytes.

generate_dataset(batchsize) yields device fp32 tensors [B, H, W, 3] = ((v / 255) - normal[0]) / normal[1] (load_images, :36-49): each batch is
decoded into one pinned uint8 buffer by a worker thread, copied up asynchronously (1, 3 or 4 bytes per pixel instead of 12) and expanded by
`cp_frames_to_input_f32` (csrc/frames.hip) on a side stream; the consumer's stream waits on an event recorded after the kernel.  There is no
CPU path.
"""
from __future__ import annotations

import collections
import glob
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np


def find_frames(root: str) -> List[str]:
    """Image paths under `root` in the reference's order (load_image_data, :51-82)."""
    imgs: List[str] = []

    def collect(path):
        files = sorted(glob.glob(os.path.join(glob.escape(path), "*[0-9].png")))
        if not files:
            files = sorted(glob.glob(os.path.join(glob.escape(path), "*[0-9].jpg")))
        imgs.extend(f for f in files if os.path.isfile(f))

    def explore(path):
        if not os.path.isdir(path):
            return
        folders = sorted(os.path.join(path, o) for o in os.listdir(path) if os.path.isdir(os.path.join(path, o)))
        if folders:
            for folder in folders:
                explore(folder)
        else:
            collect(path)

    explore(root)
    return imgs


def _raw_modes(im) -> List[str]:
    out = []
    for t in getattr(im, "tile", None) or []:
        args = t[3] if len(t) > 3 else None
        out.append(args if isinstance(args, str) else (args[0] if isinstance(args, (tuple, list)) and args and isinstance(args[0], str) else ""))
    return out


def decode_frame(path: str) -> np.ndarray:
    """uint8 [h, w, c] with c = 1, 3 or 4, as described in the module docstring; ValueError naming the file for what cannot be input."""
    from PIL import Image

    with Image.open(path) as im:
        mode = im.mode
        if mode in ("LA", "La", "PA"):
            raise ValueError("%s: two-channel image (mode %s, grey + alpha) cannot be network input; convert it to L or RGB" % (path, mode))
        if mode.startswith("I;16") or mode in ("I", "F") or any(";16" in r for r in _raw_modes(im)):
            raise ValueError("%s: 16-bit image (mode %s) cannot be network input; convert it to 8 bits per channel" % (path, mode))
        if mode == "1":
            im = im.convert("L")
        elif mode == "P":
            im = im.convert("RGBA" if "transparency" in im.info else "RGB")
        elif mode not in ("L", "RGB", "RGBA"):
            raise ValueError("%s: image mode %s is not supported (L, RGB, RGBA or a palette image)" % (path, mode))
        a = np.asarray(im, dtype=np.uint8)
    return a[..., None] if a.ndim == 2 else a


class ImageOnlyDataset:
    def __init__(self, root, normal=[0.5, 0.5]):  # noqa: B006 (the reference's signature)
        self.root = root
        self.normal = normal
        self.imgs = find_frames(root)

    def __len__(self):
        return len(self.imgs)

    def __getitem__(self, index):
        path = self.imgs[index]
        return {"path": path, "name": os.path.splitext(os.path.basename(path))[0]}

    def frame_shape(self) -> Tuple[int, int, int]:
        """(h, w, channels) of the first image: every frame must match it (create_base_dataset, :85-95)."""
        if not self.imgs:
            raise ValueError("no *[0-9].png / *[0-9].jpg frames under %s" % self.root)
        return tuple(decode_frame(self.imgs[0]).shape)

    def load_frames(self, indices: Sequence[int], shape: Optional[Tuple[int, int, int]] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """uint8 [len(indices), h, w, c] of the decoded frames (into `out` when given).  A frame whose (h, w, c) differs from `shape`
        (default: the first image's) raises ValueError naming the file -- the reference fails there through set_shape (:38)."""
        shape = tuple(shape) if shape is not None else self.frame_shape()
        if out is None:
            out = np.empty((len(indices),) + shape, np.uint8)
        for k, i in enumerate(indices):
            a = decode_frame(self.imgs[i])
            if a.shape != shape:
                raise ValueError("%s: frame is %d x %d with %d channel(s); the first frame (%s) fixed %d x %d with %d (frames are not resized)"
                                 % (self.imgs[i], a.shape[0], a.shape[1], a.shape[2], self.imgs[0], shape[0], shape[1], shape[2]))
            out[k] = a
        return out

    def generate_dataset(self, batchsize, device=None, prefetch: int = 2, workers: int = 2) -> Tuple[Iterator, float]:
        """(iterator over device fp32 [batchsize, H, W, 3] batches, epoch_batches) of one pass in file order (:84-106).  The remainder
        is dropped and epoch_batches = data_size / batchsize is a float, as in the reference.  device: a GPU (default: the current one).
        Up to `prefetch` batches are decoded ahead on `workers` threads.  Nothing touches the GPU before the first batch is requested."""
        batchsize = int(batchsize)
        if batchsize < 1:
            raise ValueError("batchsize must be positive")
        data_size = len(self.imgs) - (len(self.imgs) % batchsize)
        epoch_batches = data_size / batchsize
        return self._device_batches(batchsize, data_size // batchsize, device, max(int(prefetch), 1), max(int(workers), 1)), epoch_batches

    def _device_batches(self, batchsize: int, nbatches: int, device, prefetch: int, workers: int):
        import torch

        from .. import _lib

        if not torch.cuda.is_available():
            raise _lib.CasaposeHipError("ImageOnlyDataset.generate_dataset needs a ROCm GPU (there is no CPU fallback for the product path)")
        if nbatches == 0:
            return
        lib = _lib.load()
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        h, w, c = shape = self.frame_shape()
        n0, n1 = float(self.normal[0]), float(self.normal[1])
        stream = torch.cuda.Stream(device=dev)

        def prepare(b):
            buf = torch.empty((batchsize, h, w, c), dtype=torch.uint8, pin_memory=True)
            self.load_frames(range(b * batchsize, (b + 1) * batchsize), shape, buf.numpy())
            return buf

        pool = ThreadPoolExecutor(workers)
        pending: collections.deque = collections.deque()
        try:
            for b in range(nbatches):
                while len(pending) < prefetch and b + len(pending) < nbatches:
                    pending.append(pool.submit(prepare, b + len(pending)))
                host = pending.popleft().result()
                with torch.cuda.stream(stream):
                    src = host.to(dev, non_blocking=True)   # the pinned block is not reused before this copy completes
                    img = torch.empty((batchsize, h, w, 3), dtype=torch.float32, device=dev)
                    _lib.check(lib.cp_frames_to_input_f32(src.data_ptr(), batchsize, h, w, c, w * c, h * w * c, n0, n1, img.data_ptr(),
                                                          stream.cuda_stream), "cp_frames_to_input_f32")
                    done = torch.cuda.Event()
                    done.record(stream)
                consumer = torch.cuda.current_stream(dev)
                consumer.wait_event(done)
                img.record_stream(consumer)
                yield img
        finally:
            for f in pending:
                f.cancel()
            pool.shutdown(wait=True)


__all__ = ["ImageOnlyDataset", "decode_frame", "find_frames"]
