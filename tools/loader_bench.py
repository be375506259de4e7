"""Throughput of the training loader alone (draw -> gather -> crop/warp -> intensity augmentation) with the frames in HBM and in pinned host
memory (datasets/resident.py), on synthetic frames: python tools/loader_bench.py [--frames 20000] [--size 256] [--batch 512] [--steps 60]
[--resample bilinear|area] [--mix one|two|four]
--mix: one dataset (POSE_WITH_LANDMARKS, the default), two (+ ONLY_POSE, weights 60 : 20), or the four-Tag mix of a run over 300W-LP, Face
Synthetics, Panoptic and LaPa (POSE_WITH_LANDMARKS : ONLY_LANDMARKS_25D : ONLY_POSE : ONLY_LANDMARKS_2D = 60 : 10 : 20 : 20) - every set
with --frames / (number of sets) frames of the same size."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "neuralnet-tracker-traincode_amd"))
from trackertraincode.datasets.resident import ResidentFrames, ResidentLoader  # noqa: E402
from trackertraincode.datatransformation.gpu import GpuFocusRoiAugment  # noqa: E402
from trackertraincode.pipelines import Tag, make_image_augmentations  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20000)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--resample", choices=("bilinear", "area"), default="bilinear", help="the crop's resampler (GpuFocusRoiAugment)")
ap.add_argument("--mix", choices=("one", "two", "four"), default="one", help="how many datasets (and Tags) a step draws from")
a = ap.parse_args()
g = torch.Generator().manual_seed(0)
MIXES = {"one": [(Tag.POSE_WITH_LANDMARKS, 1.0)], "two": [(Tag.POSE_WITH_LANDMARKS, 60.0), (Tag.ONLY_POSE, 20.0)],
         "four": [(Tag.POSE_WITH_LANDMARKS, 60.0), (Tag.ONLY_LANDMARKS_25D, 10.0), (Tag.ONLY_POSE, 20.0), (Tag.ONLY_LANDMARKS_2D, 20.0)]}
LABELS = {Tag.POSE_WITH_LANDMARKS: ("coord", "pose", "pt3d_68", "shapeparam"), Tag.ONLY_POSE: ("coord", "pose"), Tag.ONLY_LANDMARKS_25D: ("pt3d_68",),
          Tag.ONLY_LANDMARKS_2D: ("pt2d_68",)}
S = a.size
N = a.frames // len(MIXES[a.mix])


def frames_of(tag):
    every = {
        "coord": lambda: torch.tensor([[0.5 * S, 0.5 * S, 0.25 * S]]).repeat(N, 1),
        "pose": lambda: torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=-1),
        "pt3d_68": lambda: torch.rand(N, 68, 3, generator=g) * S,
        "pt2d_68": lambda: torch.rand(N, 68, 2, generator=g) * S,
        "shapeparam": lambda: torch.randn(N, 50, generator=g),
    }
    fields = {
        "image": torch.randint(0, 255, (N, 1, S, S), dtype=torch.uint8, generator=g),
        "roi": torch.tensor([[0.2 * S, 0.2 * S, 0.8 * S, 0.8 * S]]).repeat(N, 1) + torch.randn(N, 4, generator=g) * 4,
    }
    fields.update((k, every[k]()) for k in LABELS[tag])
    fields["coord_convention_id"] = torch.zeros(N, dtype=torch.int32)
    return ResidentFrames(tag, fields)


host_sets = [frames_of(tag) for tag, _ in MIXES[a.mix]]
weights = [w for _, w in MIXES[a.mix]]
for placement in ("device", "host"):
    sets = [h.to("cuda") if placement == "device" else h.to_host() for h in host_sets]
    augs = make_image_augmentations(torch.Generator().manual_seed(1))
    crop = GpuFocusRoiAugment(new_size=129, rotation_aug_angle=30.0, extension_factor=1.1, whiten=False, flip_rot_p=0.01, resample=a.resample)
    loader = ResidentLoader(sets, weights, a.batch, a.steps, seed=3, crop=crop, image_augmentations=augs)
    for _ in loader:  # warm-up epoch (allocator, pinned staging buffers)
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for step in loader:
        n += sum(int(b["image"].shape[0]) for b in step)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"frames on {placement:6s} [{a.resample}, {len(sets)} set(s)]: {n / dt:10.0f} crops/s  ({dt / a.steps * 1e3:.2f} ms per batch of {a.batch}, source frames {S}x{S}, "
          f"{sum(f.nbytes() for f in sets) / 2**30:.2f} GiB)", flush=True)
