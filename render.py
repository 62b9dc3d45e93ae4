"""python render.py --cfg configs/config_mld_gimo.yaml --input recording.npz --motion motion.npz --output frames.npy [--png_dir frames/]
A recording and the motion predict.py estimated for it -> uint8 frames of both bodies and the scene cloud, rasterised in HIP
(INTEGRATION.md M); see seeme_amd/cli.py."""
from seeme_amd.cli import render_main

if __name__ == "__main__":
    render_main()
