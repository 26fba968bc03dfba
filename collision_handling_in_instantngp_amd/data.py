"""Data formats either side of the hot path, mirrored from the reference so that a training script
written against it finds the same names and conventions:

  MyDataset            utils.py:12-75      image file -> (X, Y, height, width); X = integer (row, col) pixel list in
                                           row-major order, Y = channels / 255
  normalise / permutation                  main.py:50-58: x / (max(w, h) - 1); shuffled_indices and their inverse
  ImageSampler                             (no counterpart) training batches drawn on the device from the uint8 image itself:
                                           random continuous positions with bilinear targets, or random pixel centres
  reassemble_image     functions.py:308,332-335: inverse permutation, (output * 255) -> int32 image (truncation)
  reassemble_image_device                  the same image as a device tensor, written by the scatter kernel
  save_checkpoint / load_checkpoint        functions.py:761-781, models.py HPD/encoding weight paths: the five
                                           state-dict files of the reference, loadable in either direction
  save_snapshot                            the same five files from the best state train.fit kept on the device
  save_baked / load_baked                  a train.BakedGrid (vertex grids + decoder: the picture without the model) as one file

Host-side numpy/torch only, with two exceptions: reassemble_image_device runs the image scatter kernel (csrc/metrics.hip,
through ops.image_scatter) and needs device tensors, and ImageSampler lives on the device (csrc/sample.hip, through
ops.sample_pixels)."""
import os
from typing import Optional, Tuple

import numpy as np
import torch

CHECKPOINT_FILES = {            # functions.py:768-781
    "model": "whole_model.pt",
    "optimizer": "whole_opt.pt",
    "encoding": "encoding_model.pt",
    "HPD": "HPD_model.pt",
    "mlp": "MLP_model.pt",
}


def pixel_grid(height: int, width: int) -> np.ndarray:
    """(height*width, 2) integer (row, col) of every pixel, rows outermost (utils.py:56-59: meshgrid(range(height),
    range(width), indexing='ij') flattened)."""
    rows = np.repeat(np.arange(height, dtype=np.int64), width)
    cols = np.tile(np.arange(width, dtype=np.int64), height)
    return np.stack([rows, cols], axis=1)


def to_grayscale(rgb: np.ndarray) -> np.ndarray:
    """uint8 luma with OpenCV's COLOR_BGR2GRAY weights (0.299 R + 0.587 G + 0.114 B, 14-bit fixed point, rounded)."""
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


class MyDataset(torch.utils.data.Dataset):
    """reference utils.py:12-75.  One image; `dataset[0]` -> (X float32 (P,2), Y float32 (P,C), height, width).
    The image is decoded with Pillow (cv2 is not a dependency here); `image=` takes an already decoded (H,W,3) uint8
    RGB array instead of a file."""

    def __init__(self, root: str = ".", dir_name: str = "images", image_name: str = "", should_bw: bool = False,
                 image: Optional[np.ndarray] = None) -> None:
        self._root = root
        self._dir_name = dir_name
        self._image_name = image_name
        self._should_bw = should_bw
        self._image_path = os.path.join(os.path.join(self._root, self._dir_name), self._image_name)
        self._source = None if image is None else np.asarray(image)
        self._image = None

    def _load_rgb(self) -> np.ndarray:
        if self._source is not None:
            return self._source[:, :, :3]
        from PIL import Image
        with Image.open(self._image_path) as im:
            return np.asarray(im.convert("RGB"))

    def __getitem__(self, idx: int) -> Tuple[torch.Tensor, torch.Tensor, int, int]:
        rgb = self._load_rgb()
        self._image = to_grayscale(rgb) if self._should_bw else np.ascontiguousarray(rgb)
        height, width = self._image.shape[0], self._image.shape[1]
        X = torch.from_numpy(pixel_grid(height, width)).float()
        Y = torch.from_numpy(self._image.reshape(height * width, -1).astype(np.float64) / 255).float()
        return X, Y, height, width            # height, width in this order, as the reference returns them

    def __len__(self) -> int:
        return 1

    def get_image(self) -> np.ndarray:
        return self._image

    def get_image_name(self) -> str:
        return self._image_name


def normalise_coordinates(x: torch.Tensor, w: int, h: int) -> torch.Tensor:
    """main.py:50-51: pixel indices -> [0, 1] by the longer side."""
    return x / (max(w, h) - 1)


def make_permutation(shape: int, generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """main.py:55-58: (shuffled_indices, reordered_indices) as int32, reordered[shuffled] = arange."""
    shuffled = torch.randperm(shape, generator=generator).int()
    reordered = torch.zeros((shape,)).int()
    reordered[shuffled.long()] = torch.arange(shape).int()
    return shuffled, reordered


class ImageSampler:
    """Training batches drawn on the device from the uint8 image itself (ops.sample_pixels, csrc/sample.hip) — the image task of
    Instant-NGP: `batch` random positions per draw, continuous (targets looked up bilinearly) or pixel centres with replacement.
    The image, 1 B per pixel and channel, is the only per-pixel storage: no coordinate tensor, no target tensor, no permutation.

        sampler = ImageSampler(img, 2 ** 18)             # img: uint8 (h,w) | (h,w,C <= 4), numpy or a device tensor
        x, target = sampler.next()                       # (batch,2) fp32 (row, col) / denom and (batch,C) fp32

    next() returns views of one of `buffers` rotating pairs: a batch stays valid for buffers - 1 further draws.  It does not
    allocate and does not synchronise (capturable: the draw counter lives on the device, every replay draws a new batch).
    coord_bounds: an upper bound of the coordinates of every batch (GraphedStep's coord_bounds)."""

    def __init__(self, image, batch: int, *, seed: int = 0, continuous: bool = True, denom: Optional[float] = None,
                 device="cuda", buffers: int = 2) -> None:
        img = torch.as_tensor(image)
        if img.dtype != torch.uint8:
            raise TypeError(f"image must be uint8, got {img.dtype}")
        if img.dim() == 2:
            img = img.unsqueeze(-1)
        if img.dim() != 3 or not 1 <= img.shape[2] <= 4:
            raise ValueError(f"image must be (h, w) or (h, w, C <= 4), got {tuple(img.shape)}")
        self.h, self.w, self.C = (int(s) for s in img.shape)
        self.batch, self.seed, self.continuous = int(batch), int(seed), bool(continuous)
        if self.batch < 1 or int(buffers) < 1:
            raise ValueError("batch and buffers must be at least 1")
        if self.h < 1 or self.w < 1 or (self.continuous and (self.h < 2 or self.w < 2)):
            raise ValueError(f"a {self.h} x {self.w} image cannot be sampled" + (" continuously" if self.continuous else ""))
        if denom is None:
            denom = max(self.h, self.w) - 1
        self.denom = float(denom)
        if not self.denom > 0:
            raise ValueError(f"denom must be > 0, got {self.denom} (a 1 x 1 image needs an explicit denom)")
        self.image = img.to(device).contiguous()
        dev = self.image.device
        self._draw = torch.zeros((), dtype=torch.int64, device=dev)
        self._pairs = [(torch.empty((self.batch, 2), dtype=torch.float32, device=dev),
                        torch.empty((self.batch, self.C), dtype=torch.float32, device=dev)) for _ in range(int(buffers))]
        self.buffers = len(self._pairs)
        self._turn = 0
        # the largest coordinates any draw can give, in the kernel's own fp32 arithmetic
        f32 = np.float32
        self.coord_bounds = (float(f32(self.h - 1) / f32(self.denom)), float(f32(self.w - 1) / f32(self.denom)))

    def next(self) -> Tuple[torch.Tensor, torch.Tensor]:
        from . import ops
        x, target = self._pairs[self._turn]
        self._turn = (self._turn + 1) % len(self._pairs)
        ops.sample_pixels(self.image, self.seed, self._draw, x, target, denom=self.denom, continuous=self.continuous)
        # written in place behind torch's back: whoever keys a cache on (address, version) — the binning pipeline — must see it
        torch.autograd.graph.increment_version(x)
        torch.autograd.graph.increment_version(target)
        return x, target

    @property
    def draw(self) -> int:
        """the number of batches drawn so far (reads the device counter: synchronises)"""
        return int(self._draw.item())

    def data_bytes(self) -> int:
        """device bytes of the data side: the image, the batch buffers and the counter"""
        return (self.image.numel() + 8 + sum(x.numel() * 4 + t.numel() * 4 for x, t in self._pairs))

    def state_dict(self) -> dict:
        return {"seed": self.seed, "draw": self.draw, "batch": self.batch, "mode": "continuous" if self.continuous else "pixel"}

    def load_state_dict(self, state: dict) -> None:
        """continues the sequence of draws of a sampler of the same batch size and mode (the draws depend on both)"""
        mode = "continuous" if self.continuous else "pixel"
        if int(state["batch"]) != self.batch or state["mode"] != mode:
            raise ValueError(f"state of a sampler with batch {state['batch']}, mode {state['mode']!r}; this one has {self.batch}, {mode!r}")
        self.seed = int(state["seed"])
        self._draw.fill_(int(state["draw"]))


def reassemble_image(outputs: torch.Tensor, reordered_indices: Optional[torch.Tensor], h: int, w: int,
                     should_bw: bool = False, should_shuffle: bool = True) -> np.ndarray:
    """functions.py:308,332-335: batch-order outputs -> image order -> (output * 255) as int32 (h,w,3) / (h,w)
    (torch's float -> int conversion truncates toward zero; values are not clamped, as in the reference)."""
    out = outputs[reordered_indices.long()] if should_shuffle else outputs
    img = (out * 255).reshape((h, w, 3) if not should_bw else (h, w))
    return img.int().detach().cpu().numpy()


def reassemble_image_device(outputs: torch.Tensor, reordered_indices: Optional[torch.Tensor], h: int, w: int,
                            should_bw: bool = False, should_shuffle: bool = True) -> torch.Tensor:
    """reassemble_image's result as a device int32 tensor, without the gather: with shuffled the inverse of
    reordered_indices, img[shuffled[i]] = out[i] is what the scatter kernel writes (csrc/metrics.hip).  outputs: device
    fp32, (h*w, 3) or, should_bw, h*w values."""
    from . import ops
    P = h * w
    out = outputs.detach().reshape(P, -1)
    if out.shape[1] != (1 if should_bw else 3):
        raise ValueError(f"outputs {tuple(outputs.shape)} do not fill a {(h, w) if should_bw else (h, w, 3)} image")
    out = out if out.is_contiguous() else out.contiguous()
    shuffled = None
    if should_shuffle:
        ro = reordered_indices.reshape(-1).to(out.device).long()
        # the kernel trusts its indices: reordered_indices must be a permutation of range(P)
        if ro.numel() != P or int(ro.min()) < 0 or int(ro.max()) >= P:
            raise ValueError(f"reordered_indices must be a permutation of range({P})")
        shuffled = torch.full((P,), -1, dtype=torch.int32, device=out.device)
        shuffled[ro] = torch.arange(P, dtype=torch.int32, device=out.device)
        if int(shuffled.min()) < 0:
            raise ValueError(f"reordered_indices must be a permutation of range({P})")
    img = torch.empty((P, out.shape[1]), dtype=torch.int32, device=out.device)
    ops.image_scatter(out, shuffled, img, 0)
    return img.view((h, w) if should_bw else (h, w, 3))


def save_checkpoint(net, optimizer, folder: str) -> dict:
    """functions.py:764-781: the whole model, the optimizer and the three sub-modules as separate state dicts."""
    os.makedirs(folder, exist_ok=True)
    paths = {k: os.path.join(folder, v) for k, v in CHECKPOINT_FILES.items()}
    torch.save(net.state_dict(), paths["model"])
    if optimizer is not None:
        torch.save(optimizer.state_dict(), paths["optimizer"])
    torch.save(net.encoding.state_dict(), paths["encoding"])
    if getattr(net, "HPD", None) is not None:
        torch.save(net.HPD.state_dict(), paths["HPD"])
    torch.save(net.mlp.state_dict(), paths["mlp"])
    return paths


def save_snapshot(snapshot, net, optimizer, folder: str) -> dict:
    """save_checkpoint's five files from a train.DeviceSnapshot of train.state_tensors(net, optimizer) — the best state
    fit() kept on the device — instead of the live model: same names and layouts, loadable with load_checkpoint.  net and
    optimizer give the structure (keys, parameter groups, hyper-parameters); every tensor comes from the snapshot."""
    held = snapshot.tensors()
    model = {k: held[f"model.{k}"].detach().clone() for k in net.state_dict().keys()}

    def part(prefix):
        return {k[len(prefix):]: v for k, v in model.items() if k.startswith(prefix)}

    os.makedirs(folder, exist_ok=True)
    paths = {k: os.path.join(folder, v) for k, v in CHECKPOINT_FILES.items()}
    torch.save(model, paths["model"])
    if optimizer is not None:
        sd = optimizer.state_dict()
        sd["state"] = {i: {k: (held[f"optimizer.{i}.{k}"].detach().clone() if torch.is_tensor(v) else v) for k, v in st.items()}
                       for i, st in sd["state"].items()}
        torch.save(sd, paths["optimizer"])
    torch.save(part("encoding."), paths["encoding"])
    if getattr(net, "HPD", None) is not None:
        torch.save(part("HPD."), paths["HPD"])
    torch.save(part("mlp."), paths["mlp"])
    return paths


def load_checkpoint(net, folder: str, optimizer=None, parts=("model",), map_location=None) -> None:
    """Loads `whole_model.pt` (parts=('model',)) or any of the per-module files ('encoding', 'HPD', 'mlp'), and the
    optimizer state when given.  Files written by the reference load as well: parameter names are the same."""
    for part in parts:
        state = torch.load(os.path.join(folder, CHECKPOINT_FILES[part]), map_location=map_location)
        target = net if part == "model" else getattr(net, part)
        target.load_state_dict(state)
    if optimizer is not None:
        optimizer.load_state_dict(torch.load(os.path.join(folder, CHECKPOINT_FILES["optimizer"]), map_location=map_location))


BAKED_FORMAT = "gngf-baked-grid/1"
BAKED_FIELDS = ("grid", "decoder", "n_ls_host", "L", "F", "out_dim", "leaky")      # train.BakedGrid.FIELDS


def save_baked(baked, path: str) -> None:
    """One file for a train.BakedGrid: a dict of tensors and plain numbers — the format tag, the field list and the fields
    (grid, the six decoder tensors, the level resolutions, L, F, out_dim, leaky), tensors moved to the host.  The model, its
    HPD and its tables are not needed to draw the picture again (load_baked(path).render(...))."""
    state = {"format": BAKED_FORMAT, "fields": list(BAKED_FIELDS),
             "grid": baked.grid.detach().cpu(), "decoder": [t.detach().cpu() for t in baked.decoder],
             "n_ls_host": [int(n) for n in baked.n_ls_host], "L": int(baked.L), "F": int(baked.F), "out_dim": int(baked.out_dim),
             "leaky": bool(baked.leaky)}
    torch.save(state, path)


def load_baked(path: str, device="cuda"):
    """The train.BakedGrid that save_baked wrote, on `device`.  ValueError for a file with another format tag or field list, or
    whose shapes do not fit its own numbers (grid rows for the resolutions, decoder widths for L F and out_dim)."""
    from . import train
    state = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(state, dict) or state.get("format") != BAKED_FORMAT or tuple(state.get("fields", ())) != BAKED_FIELDS:
        tag = state.get("format") if isinstance(state, dict) else type(state).__name__
        raise ValueError(f"{path} is not a baked grid of format {BAKED_FORMAT!r} (found {tag!r})")
    missing = [k for k in BAKED_FIELDS if k not in state]
    if missing:
        raise ValueError(f"{path} lacks the fields {missing}")
    if not torch.is_tensor(state["grid"]) or not all(torch.is_tensor(t) for t in state["decoder"]):
        raise ValueError(f"{path}: grid and decoder must be tensors")
    baked = train.BakedGrid(state["grid"].to(device), [t.to(device) for t in state["decoder"]], state["n_ls_host"], state["leaky"])
    if (baked.L, baked.F, baked.out_dim) != (state["L"], state["F"], state["out_dim"]):
        raise ValueError(f"{path}: tensors of L, F, out_dim = {(baked.L, baked.F, baked.out_dim)} but the file says "
                         f"{(state['L'], state['F'], state['out_dim'])}")
    return baked
