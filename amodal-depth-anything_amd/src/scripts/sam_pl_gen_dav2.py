#!/usr/bin/env python
"""ADIW pseudo-label generation: the counterpart of the reference's ``src/scripts/sam_pl_gen_dav2.py``.

The reference walks hard-wired cluster directories one sample at a time: the un-occluded SA-1B photo and the occluded composite through the raw ViT-G,
both maps min-max normalised, the first fitted onto the second over the visible mask, the fitted map pasted inside the whole mask, the result quantised
to 16 bits and saved as a 512 x 512 PNG ``{id}_depth.png`` -- the ground truth that ``amodal_dav2_inference.py --gt_depth_dir`` reads.  This runner takes
the directories as arguments, keeps the file-name patterns and the chunking (``--data_index`` selects one of ``ceil(n / chunk_size)`` parts of
``np.array_split``, lines 53-56), and hands batches of pairs to hip_ext.labels.pseudo_label_pairs: Pillow's resize, one network batch of 2 P, the fit, the
paste and the quantisation all run on the device, and only the uint16 labels come back.

    python -m src.scripts.sam_pl_gen_dav2 --image_dir A --occ_image_dir B --visible_mask_dir C --whole_mask_dir D --valid_file valid.txt \
        --data_index 0 --output_dir OUT [--raw_weights depth_anything_v2_vitg.pth] [--batch_size 8]

Decoding and ``convert('RGB')`` stay on the host.  Multi-GPU: one process per GPU as for amodal_dav2_inference.py; the chunk is sharded contiguously over
the ranks and each rank writes its own PNGs.
"""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Tuple

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(os.path.dirname(HERE))
if PKG not in sys.path:
    sys.path.insert(0, PKG)

RAW_CONFIGS = {"vits": (64, [48, 96, 192, 384]), "vitb": (128, [96, 192, 384, 768]), "vitl": (256, [256, 512, 1024, 1024]),
               "vitg": (384, [1536, 1536, 1536, 1536])}     # the script's line 60 is the last one


def read_valid_file(path: str) -> List[str]:
    """Sample ids, one per line (the script's lines 50-52); blank lines are dropped."""
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def chunk_ids(ids: List[str], data_index: int, chunk_size: int = 40000) -> List[str]:
    """Part ``data_index`` of ``np.array_split(ids, ceil(len(ids) / chunk_size))`` (lines 53-56)."""
    if not ids:
        raise ValueError("no sample ids")
    num_chunks = int(np.ceil(len(ids) / chunk_size))
    if not 0 <= data_index < num_chunks:
        raise ValueError(f"data_index {data_index} outside the {num_chunks} chunks of {len(ids)} samples at chunk_size {chunk_size}")
    return [str(s) for s in np.array_split(np.asarray(ids, dtype=object), num_chunks)[data_index]]


def sample_paths(sid: str, image_dir: str, occ_image_dir: str, visible_mask_dir: str, whole_mask_dir: str, output_dir: str) -> Dict[str, str]:
    """The files of one sample (lines 65, 79, 92, 96, 121)."""
    return dict(image=os.path.join(image_dir, f"sa_{sid}.jpg"), occ=os.path.join(occ_image_dir, f"{sid}_occlusion.png"),
                visible=os.path.join(visible_mask_dir, f"{sid}_visible_mask.png"), whole=os.path.join(whole_mask_dir, f"{sid}_whole_mask.png"),
                out=os.path.join(output_dir, f"{sid}_depth.png"))


def resample_for_mode(mode: str) -> str:
    """The filter ``Image.resize(size)`` applies to a file of this mode under the reference's Pillow: NEAREST for modes 1 and P, BICUBIC otherwise."""
    return "nearest" if mode in ("1", "P") else "bicubic"


def load_photo(path: str) -> np.ndarray:
    """``Image.open(fp).convert('RGB')`` as uint8 [h, w, 3] (load_im, line 28, before its resize)."""
    assert os.path.exists(path), f"File not found: {path}"
    return np.asarray(Image.open(path).convert("RGB"))


def load_mask(path: str) -> Tuple[np.ndarray, str]:
    """(uint8 [h, w], resample) of a mask file (lines 93, 97, before their resize).  A mask that does not decode to [h, w] (RGB, RGBA, LA) is converted to
    L first and resized as L; the reference would fail on it."""
    assert os.path.exists(path), f"File not found: {path}"
    im = Image.open(path)
    arr = np.asarray(im)
    if arr.ndim != 2:
        im = im.convert("L")
        arr = np.asarray(im)
    if arr.dtype == np.bool_:
        arr = arr.astype(np.uint8)
    if arr.dtype != np.uint8:
        raise ValueError(f"{path}: mode {im.mode} masks are not supported (8-bit, 1-bit and palette masks are)")
    return np.ascontiguousarray(arr), resample_for_mode(im.mode)


def load_sample(paths: Dict[str, str]):
    """(photo, composite, (visible mask, resample), (whole mask, resample)) of one sample, decoded on the host."""
    return load_photo(paths["image"]), load_photo(paths["occ"]), load_mask(paths["visible"]), load_mask(paths["whole"])


def save_label(label: np.ndarray, path: str) -> None:
    """uint16 [h, w] -> a 16-bit PNG (line 121's save)."""
    Image.fromarray(label).save(path)


def run(model_raw: Callable, ids: List[str], image_dir: str, occ_image_dir: str, visible_mask_dir: str, whole_mask_dir: str, output_dir: str,
        batch_size: int = 8, size: int = 518, label_size: int = 512, overflow: str = "wrap", group=None, decode_workers: int = 8) -> Dict[str, int]:
    """Writes ``{output_dir}/{id}_depth.png`` (mode I;16) for every id and returns dict(samples, out_of_range): the samples written and how many of them
    had a label pixel whose value * 65535 left [0, 65536) -- wrapped by the reference's cast -- summed over the ranks.  ``decode_workers`` host threads
    decode the next batch and encode the finished labels while the device works."""
    from hip_ext.labels import pseudo_label_pairs
    os.makedirs(output_dir, exist_ok=True)
    import torch.distributed as dist
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    if world > 1:   # this rank's contiguous share of the chunk
        from hip_ext.parallel import shard_range
        lo, hi = shard_range(len(ids), dist.get_rank(group), world)
        ids = ids[lo:hi]
    flagged = 0
    batches = [ids[i:i + batch_size] for i in range(0, len(ids), batch_size)]
    # decoding four files per sample is most of a pass (profiles/pseudo_label.txt): the next batch is decoded, and the labels of the last one are
    # encoded, by host threads while the device works on this one (Pillow releases the interpreter lock inside its codecs)
    with ThreadPoolExecutor(max_workers=max(int(decode_workers), 1)) as pool:
        def submit(batch):
            paths = [sample_paths(s, image_dir, occ_image_dir, visible_mask_dir, whole_mask_dir, output_dir) for s in batch]
            return paths, [pool.submit(load_sample, p) for p in paths]
        ahead = submit(batches[0]) if batches else None
        saves = []
        for k in range(len(batches)):
            paths, loads = ahead
            ahead = submit(batches[k + 1]) if k + 1 < len(batches) else None
            samples = [f.result() for f in loads]
            res = pseudo_label_pairs(model_raw, [s[0] for s in samples], [s[1] for s in samples], [s[2][0] for s in samples], [s[3][0] for s in samples],
                                     size=size, label_size=label_size, overflow=overflow, mask_resample=[(s[2][1], s[3][1]) for s in samples])
            labels = res.label.cpu().numpy()
            flagged += int((res.out_of_range.cpu() != 0).sum())
            saves += [pool.submit(save_label, arr, p["out"]) for p, arr in zip(paths, labels)]
        for f in saves:
            f.result()
    totals = [len(ids), flagged]
    if world > 1:
        dev = next(model_raw.parameters()).device
        vec = torch.tensor(totals, dtype=torch.int64, device=dev if dist.get_backend(group) == "nccl" else "cpu")
        dist.all_reduce(vec, group=group)
        totals = vec.tolist()
    return dict(samples=int(totals[0]), out_of_range=int(totals[1]))


def load_model(encoder: str, raw_weights, device):
    from src.models.amodalsynthdrive.depth_anything_v2_raw.dpt import DepthAnythingV2
    features, out_channels = RAW_CONFIGS[encoder]
    model = DepthAnythingV2(encoder=encoder, features=features, out_channels=out_channels)
    if raw_weights:
        model.load_state_dict(torch.load(raw_weights, map_location="cpu"), strict=False)      # line 61
    else:   # no checkpoints ship with this repository: deterministic synthetic weights keep the runner usable end to end
        from src.util.synth_weights import fill_state_dict_
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        fill_state_dict_(sd, 0)
        model.load_state_dict(sd, strict=True)
    return model.eval().to(device)


def main(argv=None):
    ap = argparse.ArgumentParser(description="ADIW pseudo-label generation on the device (MI355X-native HIP path)")
    ap.add_argument("--image_dir", required=True, help="un-occluded photos, sa_{id}.jpg")
    ap.add_argument("--occ_image_dir", required=True, help="occluded composites, {id}_occlusion.png")
    ap.add_argument("--visible_mask_dir", required=True, help="{id}_visible_mask.png")
    ap.add_argument("--whole_mask_dir", required=True, help="{id}_whole_mask.png.  Masks of mode 1 or P are resized with NEAREST, every other with BICUBIC, "
                    "as Pillow does; a mask that does not decode to [h, w] (RGB, RGBA) is converted to L first -- the reference would fail on it")
    ap.add_argument("--valid_file", required=True, help="text file, one sample id per line")
    ap.add_argument("--data_index", type=int, default=0, help="which chunk of the id list to process")
    ap.add_argument("--chunk_size", type=int, default=40000, help="the list is cut into ceil(n / chunk_size) parts by np.array_split")
    ap.add_argument("--output_dir", required=True, help="{id}_depth.png, 16-bit (mode I;16)")
    ap.add_argument("--raw_weights", default=None, help="depth_anything_v2_{encoder}.pth; synthetic weights when absent")
    ap.add_argument("--encoder", default="vitg", choices=sorted(RAW_CONFIGS))
    ap.add_argument("--batch_size", type=int, default=8, help="pairs per network batch (the batch holds twice as many images)")
    ap.add_argument("--decode_workers", type=int, default=8, help="host threads that decode the next batch and encode finished labels while the device works")
    ap.add_argument("--label_size", type=int, default=512)
    ap.add_argument("--overflow", choices=("wrap", "clip"), default="wrap",
                    help="wrap: the reference's cast (numpy's astype(np.uint16): values outside [0, 65536) wrap around); clip: clamp them")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:   # one process per GPU; the process group is created before anything touches the device
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        a.device = f"cuda:{local}"
        dist.init_process_group("nccl", device_id=torch.device(a.device))
    model = load_model(a.encoder, a.raw_weights, a.device)
    ids = chunk_ids(read_valid_file(a.valid_file), a.data_index, a.chunk_size)
    res = run(model, ids, a.image_dir, a.occ_image_dir, a.visible_mask_dir, a.whole_mask_dir, a.output_dir, batch_size=a.batch_size,
              label_size=a.label_size, overflow=a.overflow, decode_workers=a.decode_workers)
    if rank == 0:
        print(f"chunk {a.data_index}: wrote {res['samples']} labels to {a.output_dir}" + (f" ({world} ranks)" if world > 1 else "") +
              f"; {res['out_of_range']} sample(s) with values outside [0, 65536) before the cast ({a.overflow})")
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
