"""Full-resolution transfer from the command line: every file under every class (or every row of a signal file), written at the
photograph's own size (``wu.infer_driver.fullres_sweep_to_dir``).

    python -m wu.fullres --checkpoint CKPT --out DIR --classes sunny,cloudy,rain [--size S] [--r R] [--eps E] [--png | --png-lz77] FILES...
    python -m wu.fullres --checkpoint CKPT --out DIR --signals FILE.npy [...] FILES...

``--r`` / ``--eps``: the guided filter's window radius (low-resolution pixels) and regulariser (``wu.guided``); the defaults are untuned."""
import argparse

import torch


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m wu.fullres", description="conditional transfer written at each photograph's own size")
    ap.add_argument("--checkpoint", required=True, help="a reference-format checkpoint (wu.infer_driver.load_checkpoint)")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--classes", help="comma-separated class names: one output per file and class")
    ap.add_argument("--signals", help=".npy file of conditioning rows (R, nc): one output per file and row, instead of the class sweep")
    ap.add_argument("--src-labels", help="comma-separated class index of every file (class sweep: the first part of the output names)")
    ap.add_argument("--size", type=int, default=224, help="the network's input size")
    ap.add_argument("--r", type=int, default=4, help="guided filter radius in low-resolution pixels (untuned default)")
    ap.add_argument("--eps", type=float, default=1e-3, help="guided filter regulariser (untuned default)")
    ap.add_argument("--png", action="store_true", help="write lossless .png files (GPU encoder) instead of .jpg")
    ap.add_argument("--png-lz77", action="store_true", help="--png with LZ77 matching: smaller files where skies clip or ramps are smooth, "
                    "never larger ones; more GPU time per file")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("files", nargs="+")
    args = ap.parse_args(argv)
    if (args.classes is None) == (args.signals is None):
        ap.error("exactly one of --classes and --signals")
    import cunet
    from . import infer_driver as D
    from .guided import GuidedUpsampler
    rows = names = None
    if args.signals is not None:
        import numpy as np
        rows = torch.from_numpy(np.load(args.signals).astype("float32")).to(args.device)
        if rows.dim() != 2:
            ap.error(f"--signals: rows (R, nc), got {tuple(rows.shape)}")
        nc, class_names, labels = rows.shape[1], None, None
    else:
        class_names = args.classes.split(",")
        nc = len(class_names)
        labels = [int(v) for v in args.src_labels.split(",")] if args.src_labels else None
    net = cunet.Conditional_UNet(nc, precision=args.precision)
    D.load_checkpoint(args.checkpoint, inference=net)
    net = net.to(args.device).eval()
    png = None
    args.png = args.png or args.png_lz77
    if args.png:
        from .png_enc import GPUPngEncoder
        png = GPUPngEncoder(device=args.device, matching="lz77" if args.png_lz77 else "none")
    with torch.cuda.device(args.device):
        written = D.fullres_sweep_to_dir(net, args.files, labels, class_names, args.out, args.size, ".png" if args.png else ".jpg",
                                         png_encoder=png, rows=rows, row_names=names, upsampler=GuidedUpsampler(args.r, args.eps))
    if png is not None:
        png.close()
    print(f"wrote {len(written)} files to {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
