"""python estimate.py --cfg <config> --checkpoint <ckpt> --input rec.npz --output rec_with_interactee.npz
A recording without the interactee (video, box, camera path, scene) -> one predict.py accepts; see seeme_amd/cli.py."""
from seeme_amd.cli import estimate_main

if __name__ == "__main__":
    estimate_main()
