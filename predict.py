"""python predict.py --cfg configs/config_mld_gimo.yaml --checkpoint <ckpt> --input recording.npz --output motion.npz
A recording without wearer labels -> one stitched SMPL motion of the wearer; see seeme_amd/cli.py."""
from seeme_amd.cli import predict_main

if __name__ == "__main__":
    predict_main()
