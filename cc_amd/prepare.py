"""python -m cc_amd.prepare: the reference's data/prepare_train_data.py (its options, with their names, types and defaults) on
cc_amd/datasets/prepare.py -- a KITTI raw or Cityscapes download -> sequence folders, the train / val lists and, with
--store-cache, the device stores' caches `python -m cc_amd.train --store-cache` starts from.

    python -m cc_amd.prepare KITTI_RAW --dataset-format kitti --test-scenes test_scenes.txt --static-frames static_frames.txt \\
        --with-gt --dump-root DUMP --height 256 --width 832 --num-threads 16 --store-cache CACHE
    python -m cc_amd.prepare CITYSCAPES --dataset-format cityscapes --dump-root DUMP --height 171 --width 416

Driver-only flags: --test-scenes FILE (required for kitti; the reference reads the list beside its script, this driver ships none;
the word `none` excludes nothing), --store-cache DIR, --sequence-length (5; the stores' samples), --device (cuda; cpu = the x86
emulation build), --chunk-frames (64 frames per upload).  One JSON line on stdout at the end."""
import argparse
import json
import sys


def build_parser():
    p = argparse.ArgumentParser(prog="python -m cc_amd.prepare", description="KITTI raw / Cityscapes -> sequence folders and stores")
    p.add_argument("dataset_dir", metavar='DIR', help='path to original dataset')
    p.add_argument("--dataset-format", type=str, required=True, choices=["kitti", "cityscapes"])
    p.add_argument("--static-frames", default=None,
                   help="list of imgs to discard for being static, if not set will discard them based on speed "
                        "(careful, on KITTI some frames have incorrect speed)")
    p.add_argument("--with-gt", action='store_true',
                   help="If available (e.g. with KITTI), will store ground truth along with images, for validation")
    p.add_argument("--dump-root", type=str, required=True, help="Where to dump the data")
    p.add_argument("--height", type=int, default=128, help="image height")
    p.add_argument("--width", type=int, default=416, help="image width")
    p.add_argument("--num-threads", type=int, default=4, help="number of threads to use")
    g = p.add_argument_group("driver")
    g.add_argument("--test-scenes", default=None, metavar='FILE',
                   help="kitti: the drives to leave out, one name per line (required; `none` excludes nothing)")
    g.add_argument("--store-cache", default=None, metavar='DIR', help="also write the stores cc_amd.train --store-cache loads")
    g.add_argument("--sequence-length", type=int, default=5, help="sequence length of the stores' samples")
    g.add_argument("--device", default='cuda', help='cuda, or cpu (the x86 emulation build)')
    g.add_argument("--chunk-frames", type=int, default=64, help="frames per upload")
    return p


def make_loader(p, args):
    from .datasets import prepare as P
    if args.dataset_format == 'kitti':
        if args.test_scenes is None:
            p.error("--dataset-format kitti needs --test-scenes FILE (the drives to leave out; `--test-scenes none` excludes nothing)")
        if args.test_scenes == 'none':
            print("=> --test-scenes none: no drive is left out, the evaluation drives included", file=sys.stderr)
        return P.KittiRaw(args.dataset_dir, [] if args.test_scenes == 'none' else args.test_scenes, static_frames=args.static_frames,
                          height=args.height, width=args.width, get_gt=args.with_gt)
    return P.Cityscapes(args.dataset_dir, height=args.height, width=args.width)


def main(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    loader = make_loader(p, args)
    from .datasets import prepare as P
    print('Retrieving frames', file=sys.stderr)
    rec = P.prepare(loader, args.dump_root, store_cache=args.store_cache, sequence_length=args.sequence_length, device=args.device,
                    workers=args.num_threads, chunk_frames=args.chunk_frames)
    print(json.dumps({"scenes": len(rec['scenes']), "frames": sum(len(v) for v in rec['frames'].values()), "train": len(rec['train']),
                      "val": len(rec['val']), "stores": rec['stores'], "seconds": {k: round(v, 4) for k, v in rec['seconds'].items()}}))
    return rec


if __name__ == "__main__":
    main()
