"""image_crops_<split>.npy / image_crop_names_<split>.npy for a dataset root and a folder of frames: the 224 x 224
patch around the interactee of every frame the split's sequence files name, cut by seeme_crop_patches (crops.write_crop_files).

    python scripts/make_image_crops.py --root datasets/EgoBody/our_process_smpl_split --frames datasets/EgoBody --split train

The patch is this package's integer definition of the reference's cv2.warpAffine call.  The frames are decoded with
PIL, which is imported here and only here: the package itself gains no dependency.  NOT MEASURED: whether PIL and OpenCV (which the
reference decodes with) turn a JPEG into the same bytes -- both build on libjpeg, but versions and IDCT settings may differ by a
grey level in some pixels.  Without a ROCm device (--device cpu) the plain-torch twin cuts the same bytes, slowly."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seeme_amd import crops as CR  # noqa: E402
from seeme_amd.data import load_pickled  # noqa: E402


def split_entries(root: str, split: str):
    """(image name, center, scale) of every frame of the split's sequence files (``recording_utils``)."""
    d = os.path.join(root, split)
    for name in sorted(n for n in os.listdir(d) if n.endswith(".npy")):
        ru = load_pickled(os.path.join(d, name))["recording_utils"]
        yield from zip((str(n) for n in ru["original_imgname"]), np.asarray(ru["center"], np.float32), np.asarray(ru["scale"], np.float32))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--root", required=True, help="dataset root: <root>/<split>/*.npy sequence files; the crop files are written here")
    p.add_argument("--frames", required=True, help="folder the image names of recording_utils.original_imgname are relative to")
    p.add_argument("--split", required=True, action="append", help="train, val or test; may be given more than once")
    p.add_argument("--device", default="cuda:0", help="ROCm device of the kernel, or cpu for the plain-torch twin")
    p.add_argument("--batch", type=int, default=64, help="frames of equal size per launch")
    args = p.parse_args(argv)
    from PIL import Image                                              # the decoder: a dependency of this script alone

    def read_frame(name):
        with Image.open(os.path.join(args.frames, name)) as im:        # (no EXIF rotation: cv2.IMREAD_IGNORE_ORIENTATION)
            return np.asarray(im.convert("RGB"), np.uint8)

    device = None if args.device == "cpu" else torch.device(args.device)
    for split in args.split:
        res = CR.write_crop_files(split_entries(args.root, split), read_frame, args.root, split, device=device, batch=args.batch)
        print(f"{split}: {res['count']} crops in {res['launches']} launches -> {res['crops']}, {res['names']}")


if __name__ == "__main__":
    main()
