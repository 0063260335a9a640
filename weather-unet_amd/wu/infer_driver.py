"""Checkpoint interchange and the inference sweep of the reference's drivers.

* Checkpoints: the reference saves ``{'inference': G.state_dict(), 'discriminator': D.state_dict(), 'epoch',
  'global_step'}`` as ``{save_dir}/{name}/{name}_e{epoch:04d}_s{step}.pt`` (t_est_train.py:365-373) and resumes
  from the lexicographically last file (t_cls_train.py:158-166).  ``save_checkpoint`` / ``load_checkpoint`` /
  ``latest_checkpoint`` reproduce that format with the same keys and OIHW fp32 tensors, so files interchange with
  the reference in both directions.  Loading uses ``weights_only=True`` (tensors and plain containers only).
* Inference: ``inference/inf_transfer_c.py:108-121`` runs, per batch, one forward per class with a tiled one-hot
  row and saves each output with ``save_image(..., normalize=True)`` (per-image min-max).  ``class_sweep`` is that
  loop on GPU tensors; ``signal_sweep`` the same loop over arbitrary conditioning rows (``inf_transfer_e.py:136-143``),
  ``transfer_rows`` the one-row-per-image call of ``inf_1year_signals.py:98-107`` (``image_rows``: one image under many rows), ``axis_sweep``
  the conditioning schedule of ``demo.py:67-82``; each takes ``shared_encoder=True`` to compute the encoder once (``Conditional_UNet.sweep``); ``normalize_minmax`` / ``to_uint8`` are save_image's arithmetic, done on the GPU.
* Writing: every one of those scripts ends in ``save_image(output, '....jpg', normalize=True)`` -- one Pillow ``Image.save`` per
  image.  ``save_images`` is that call for a batch: min-max normalisation on the GPU, then ``wu.jpeg_enc.GPUJpegEncoder`` for
  ``.jpg`` / ``.jpeg`` paths (the files are encoded on the GPU, byte for byte what Pillow writes; only the compressed bytes cross to
  the host) and Pillow for any other format -- or, for ``.png`` paths, a ``wu.png_enc.GPUPngEncoder`` passed as ``png_encoder``
  (lossless files encoded on the GPU; without one, PNG stays on Pillow).  ``class_sweep_to_dir`` is the whole loop of ``inf_transfer_c.py:114-121`` with its
  file names.
* Pictures of several images: the reference builds them with ``make_grid(..., normalize=True, scale_each=True)`` (demo.py:74-82, the
  evaluation summary of t_cls_train.py:361-378).  ``save_grid`` is ``save_image`` called with a batch, ``demo_frames`` / ``save_demo`` the
  tables and the GIF of demo.py:67-92; the composition runs on the GPU (``wu.grid``) and hands uint8 frames to the encoders.
"""
import glob
import os

import torch


def save_checkpoint(save_dir, name, inference, discriminator, epoch, global_step):
    os.makedirs(os.path.join(save_dir, name), exist_ok=True)
    path = os.path.join(save_dir, name, f"{name}_e{epoch:04d}_s{global_step}.pt")
    state = {"inference": {k: v.detach().cpu() for k, v in inference.state_dict().items()},
             "discriminator": {k: v.detach().cpu() for k, v in discriminator.state_dict().items()},
             "epoch": int(epoch), "global_step": int(global_step)}
    torch.save(state, path)
    return path


def latest_checkpoint(save_dir, name):
    """t_cls_train.py:158-160: sorted(glob(dir/*))[-1], or None."""
    found = sorted(glob.glob(os.path.join(save_dir, name, "*")))
    return found[-1] if found else None


def load_checkpoint(path, inference=None, discriminator=None, map_location="cpu"):
    """Load a reference-format checkpoint; returns (epoch, global_step).  Either module may be None."""
    sd = torch.load(path, map_location=map_location, weights_only=True)
    if inference is not None:
        inference.load_state_dict(sd["inference"])
    if discriminator is not None:
        discriminator.load_state_dict(sd["discriminator"])
    return int(sd.get("epoch", 0)), int(sd.get("global_step", 0))


def normalize_minmax(images, eps=1e-5):
    """torchvision.utils.save_image(tensor, normalize=True) as the inference scripts call it -- on ONE (3,H,W) image at a time
    (inf_transfer_c.py:118-120), i.e. per-image min-max -- with the arithmetic of the pinned torchvision (<0.4, Pipfile:11;
    utils.make_grid.norm_ip): clamp to [min, max], then (x - min) / (max - min + 1e-5).  On the GPU, whole batch at once."""
    flat = images.reshape(images.shape[0], -1)
    lo = flat.min(dim=1).values.view(-1, 1, 1, 1)
    hi = flat.max(dim=1).values.view(-1, 1, 1, 1)
    return ((images - lo) / (hi - lo + eps)).clamp_(0, 1)


def to_uint8(images01):
    """The byte image save_image writes (torchvision <0.4: ``grid.mul(255).clamp(0, 255).byte()`` -- truncation, no +0.5),
    NHWC uint8 on the GPU.  (``save_images`` does not need it: the JPEG encoder applies the same arithmetic to the float batch.)"""
    return images01.mul(255).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _run(transfer, batch, labels, graphed):
    return graphed(batch, labels, copy_out=True) if graphed is not None else transfer(batch, labels)


def _sweep(transfer, batch, rows, graphed, max_images):
    """The shared-encoder form of the loops below: ``transfer.sweep`` (or a ``GraphedSweep`` captured for this batch and row shape).
    ``max_images=None`` here means ONE ROW PER DECODER CHUNK (the batch size): every chunk is then a forward of batch B, exactly the call the
    loop makes -- same AdaIN split counts, same seed draws, so the same bits at every shape.  A larger value runs several rows per chunk (fewer,
    larger launches); the result is then that of the repeated-batch forward (``Conditional_UNet.sweep``), whose instance statistics fold their
    partial sums in an order that depends on the batch (wu_adain_stats) and can differ from the loop's in the last bits."""
    if graphed is not None:
        if not hasattr(graphed, "rows"):
            raise ValueError("shared_encoder=True needs a wu.graph_infer.GraphedSweep as `graphed`, not a GraphedUNet")
        return graphed(batch, rows, copy_out=True)
    return transfer.sweep(batch, rows, batch.shape[0] if max_images is None else max_images)


def _normalize_all(out, normalize):
    return normalize_minmax(out.reshape(-1, *out.shape[-3:])).view(out.shape) if normalize else out


@torch.no_grad()
def signal_sweep(transfer, batch, rows, normalize=False, graphed=None, shared_encoder=False, max_images=None):
    """inference/inf_transfer_e.py:136-143 (and t_cls_train.py:336-337): for every conditioning row r of ``rows`` (R, nc) --
    soft labels, standardised weather signals, scaled one-hot rows --, ``transfer(batch, r tiled B times)``.
    Returns (R, B, 3, H, W).  ``graphed``: a ``GraphedUNet`` captured for this batch shape (one hipGraph replay per row).
    The reference never calls ``.eval()`` in these scripts, so its Dropout(0.3) is active; whether this sweep uses dropout
    follows ``transfer.training`` exactly as there.
    ``shared_encoder=True``: one ``transfer.sweep`` instead of R forwards -- the encoder runs once for the batch (``graphed``: a
    ``GraphedSweep``, best captured with ``max_images=B``).  With the default ``max_images`` (one row per decoder chunk) the result is
    bit-identical to the loop's in eval mode, and with dropout active each chunk draws the seeds and masks the loop's call would.  A larger
    ``max_images`` puts several rows in one chunk: the masks are then those of the repeated-batch forward (``Conditional_UNet.sweep``), not
    those of R separate calls, and the AdaIN statistics may differ from the loop's in the last bits (see ``_sweep``)."""
    bs = batch.shape[0]
    rows = rows.to(device=batch.device, dtype=torch.float32)
    if shared_encoder:
        return _normalize_all(_sweep(transfer, batch, rows, graphed, max_images), normalize)
    outs = []
    for i in range(rows.shape[0]):
        labels = rows[i].unsqueeze(0).expand(bs, rows.shape[1]).contiguous()        # torch.cat([row] * bs).view(-1, nc)
        out = _run(transfer, batch, labels, graphed)
        outs.append(normalize_minmax(out) if normalize else out)
    return torch.stack(outs)


@torch.no_grad()
def class_sweep(transfer, batch, num_classes=None, normalize=False, graphed=None, shared_encoder=False, max_images=None):
    """inf_transfer_c.py:114-121: for every class i, ``transfer(batch, onehot[i] tiled)`` -- ``signal_sweep`` over the rows
    of the identity.  (The script's loop runs ``for i in range(bs)`` over ``onehot[i]``, i.e. it assumes batch_size ==
    num_classes; this sweep always covers all classes.)  Returns (num_classes, B, 3, H, W).  ``shared_encoder``: see ``signal_sweep``."""
    nc = num_classes if num_classes is not None else transfer.adain1.num_classes
    return signal_sweep(transfer, batch, torch.eye(nc, device=batch.device), normalize, graphed, shared_encoder, max_images)


@torch.no_grad()
def transfer_rows(transfer, batch, signals, normalize=False, graphed=None):
    """inference/inf_1year_signals.py:98-107: one conditioning row PER IMAGE (``transfer(batch, sig)``)."""
    out = _run(transfer, batch, signals.to(device=batch.device, dtype=torch.float32).contiguous(), graphed)
    return normalize_minmax(out) if normalize else out


@torch.no_grad()
def image_rows(transfer, image, signals, normalize=False, graphed=None, max_images=None):
    """inference/inf_1year_signals.py:98-107 for ONE photograph under many conditioning rows (a year of weather records): ``image`` (3, H, W)
    or (1, 3, H, W), ``signals`` (R, nc); returns (R, 3, H, W), row r = ``transfer(image, signals[r])``.  The encoder is computed once, the
    decoder runs in chunks of ``max_images`` rows (default: ``Conditional_UNet.sweep``'s; ``graphed``: a ``GraphedSweep`` of batch 1 and R
    rows).  This equals ``transfer_rows`` on the repeated image, chunk by chunk, bit for bit (in one chunk when the rows fit); with dropout
    active the masks are those of that repeated-batch forward."""
    if image.dim() == 3:
        image = image.unsqueeze(0)
    if image.dim() != 4 or image.shape[0] != 1:
        raise ValueError(f"image_rows: one image, (3, H, W) or (1, 3, H, W), got {tuple(image.shape)}")
    signals = signals.to(device=image.device, dtype=torch.float32)
    out = (graphed(image, signals, copy_out=True) if graphed is not None else transfer.sweep(image, signals, max_images))[:, 0]
    return normalize_minmax(out) if normalize else out


@torch.no_grad()
def axis_sweep(transfer, batch, pred, thetas, alpha=1.0, graphed=None, shared_encoder=False, max_images=None):
    """demo.py:67-82: for every angle theta and every class axis a, condition on the estimator's prediction ``pred`` (B, nc)
    with component a replaced by ``alpha * sin(theta)``:  c = onehot[a] * sin(theta) * alpha + (1 - onehot[a]) * pred.
    Returns (T, nc, B, 3, H, W) raw outputs (the script then maps (x + 1) * 127.5 and normalises per image for the GIF).
    ``shared_encoder=True``: the T * nc conditionings (each a row per image) go through one ``transfer.sweep`` -- see ``signal_sweep``."""
    nc = pred.shape[1]
    eye = torch.eye(nc, device=batch.device)
    pred = pred.to(device=batch.device, dtype=torch.float32)
    if shared_encoder:
        conds = []
        for theta in thetas:
            s = torch.sin(torch.as_tensor(float(theta), dtype=torch.float32, device=batch.device)) * alpha
            conds.extend(eye[a].unsqueeze(0) * s + (1.0 - eye[a]).unsqueeze(0) * pred for a in range(nc))
        out = _sweep(transfer, batch, torch.stack(conds), graphed, max_images)              # rows (T * nc, B, nc)
        return out.view(len(conds) // nc, nc, *out.shape[1:])
    frames = []
    for theta in thetas:
        s = torch.sin(torch.as_tensor(float(theta), dtype=torch.float32, device=batch.device)) * alpha
        per_axis = []
        for a in range(nc):
            c = eye[a].unsqueeze(0) * s + (1.0 - eye[a]).unsqueeze(0) * pred               # :76-79
            per_axis.append(_run(transfer, batch, c.contiguous(), graphed))
        frames.append(torch.stack(per_axis))
    return torch.stack(frames)


_default_encoder = None


def _encoder(images):
    """One shared GPUJpegEncoder with Pillow's defaults (quality 75, 4:2:0), created on first use."""
    global _default_encoder
    if _default_encoder is None or _default_encoder.device != images.device:
        from .jpeg_enc import GPUJpegEncoder
        _default_encoder = GPUJpegEncoder(device=images.device)
    return _default_encoder


def _pillow_save(arg):
    from PIL import Image
    rgb, path = arg
    Image.fromarray(rgb).save(path)


def _route_async(x, paths, encoder, png_encoder, to_bytes):
    """One batch to its files by extension: .jpg / .jpeg to ``encoder`` (default: the shared one), .png to ``png_encoder`` when one is
    passed, anything else to Pillow from ``to_bytes(sub-batch)``, an (n, H, W, 3) uint8 batch.  ``x``: whatever the encoders take, the
    float (B, 3, H, W) batch or finished (B, H, W, 3) uint8.  Returns Futures still to be waited for (Pillow's files are written)."""
    jpg = [i for i, p in enumerate(paths) if p.lower().endswith((".jpg", ".jpeg"))]
    png = [i for i, p in enumerate(paths) if p.lower().endswith(".png")] if png_encoder is not None else []
    other = [i for i in range(len(paths)) if i not in set(jpg) | set(png)]
    pending = []
    if png:
        pending.append(png_encoder.save_batch_async(x if len(png) == len(paths) else x[png], [paths[i] for i in png]))
    if jpg:
        enc = encoder if encoder is not None else _encoder(x)
        pending.append(enc.save_batch_async(x if len(jpg) == len(paths) else x[jpg], [paths[i] for i in jpg]))
    if other:
        rgb = to_bytes(x[other]).cpu().numpy()
        for k, i in enumerate(other):
            _pillow_save((rgb[k], paths[i]))
    return pending


def _save_images_async(images, paths, normalize, encoder, png_encoder=None):
    """Launch the writing of one batch; returns Futures still to be waited for (the Pillow formats are written before it returns)."""
    paths = [os.fspath(p) for p in paths]
    if images.dim() != 4 or images.shape[1] != 3 or len(paths) != images.shape[0]:
        raise ValueError(f"save_images: a (B,3,H,W) batch and B paths, got {tuple(images.shape)} and {len(paths)} paths")
    x = normalize_minmax(images.float()) if normalize else images
    return _route_async(x, paths, encoder, png_encoder, to_uint8)


@torch.no_grad()
def save_images(images, paths, normalize=True, encoder=None, png_encoder=None):
    """``[save_image(x, p, normalize=normalize) for x, p in zip(images, paths)]`` of the inference scripts for a (B, 3, H, W) batch
    on the GPU: per-image min-max (``normalize_minmax``), then bytes as ``to_uint8`` makes them.  Paths ending in .jpg / .jpeg are
    encoded by ``encoder`` (a ``GPUJpegEncoder``; default: a shared one with Pillow's defaults) from the float batch itself; any other
    format is written by Pillow from ``to_uint8``.  Either way the file equals
    ``Image.fromarray(to_uint8(normalize_minmax(x))[i]).save(path)`` byte for byte.  ``png_encoder`` (a ``wu.png_enc.GPUPngEncoder``;
    default None: Pillow, as before) takes the paths ending in .png: those files are then encoded on the GPU as well -- lossless, the
    same pixels, not Pillow's bytes.  The files exist when this returns."""
    for f in _save_images_async(images, paths, normalize, encoder, png_encoder):
        f.result()
    return [os.fspath(p) for p in paths]


@torch.no_grad()
def class_sweep_to_dir(transfer, batch, stems, src_labels, class_names, out_dir, normalize=True, graphed=None, encoder=None, ext=".jpg",
                       shared_encoder=False, max_images=None, png_encoder=None):
    """inf_transfer_c.py:114-121 down to the files: for every target class i, ``transfer(batch, onehot[i] tiled)`` and one file per
    image j named ``{class_names[src_labels[j]]}_{stems[j]}_{class_names[i]}.jpg`` (``stems[j]``: the source file's name without
    directory and extension, :120).  The files of class i are copied out and written in the background while the forward of class
    i + 1 runs (at most two classes in flight); all of them exist when this returns.  Returns the paths, target class by target class.
    ``shared_encoder=True``: all classes come from one ``transfer.sweep`` (see ``signal_sweep``), then the files are written class by class.
    ``png_encoder``: with ``ext=".png"``, the ``GPUPngEncoder`` that writes the files (see ``save_images``); None: Pillow."""
    nc = len(class_names)
    if len(stems) != batch.shape[0] or len(src_labels) != batch.shape[0]:
        raise ValueError("class_sweep_to_dir: one stem and one source label per image")
    os.makedirs(out_dir, exist_ok=True)
    rows = torch.eye(nc, device=batch.device)
    written, in_flight = [], []
    swept = _sweep(transfer, batch, rows, graphed, max_images) if shared_encoder else None
    for i in range(nc):
        out = swept[i] if shared_encoder else signal_sweep(transfer, batch, rows[i:i + 1], False, graphed)[0]
        paths = [os.path.join(out_dir, f"{class_names[int(src_labels[j])]}_{stems[j]}_{class_names[i]}{ext}") for j in range(batch.shape[0])]
        in_flight.append(_save_images_async(out, paths, normalize, encoder, png_encoder))
        written += paths
        if len(in_flight) > 2:
            for f in in_flight.pop(0):
                f.result()
    for fs in in_flight:
        for f in fs:
            f.result()
    return written


def _save_u8_async(frames, paths, encoder, png_encoder):
    """``_save_images_async`` for finished bytes: an (N, H, W, 3) uint8 batch on the GPU, routed by extension the same way."""
    return _route_async(frames, paths, encoder, png_encoder, lambda u8: u8)


@torch.no_grad()
def save_grid(tensor, path, nrow=8, padding=2, normalize=False, value_range=None, scale_each=False, pad_value=0.0, encoder=None,
              png_encoder=None):
    """``torchvision.utils.save_image(tensor, path, nrow, padding, normalize, range, scale_each, pad_value)`` for a batch: the grid of
    ``wu.grid.make_grid`` composed straight to the bytes ``to_uint8`` makes, then written as ``save_images`` writes: .jpg / .jpeg by
    ``encoder`` (a ``GPUJpegEncoder``; default: the shared one), .png by ``png_encoder`` when one is passed, else -- and any other
    format -- by Pillow.  The file exists when this returns."""
    from . import grid
    path = os.fspath(path)
    u8 = grid.compose_grid(tensor, nrow, padding, normalize, value_range, scale_each, pad_value, out="uint8").unsqueeze(0)
    for f in _save_u8_async(u8, [path], encoder, png_encoder):
        f.result()
    return path


@torch.no_grad()
def demo_frames(transfer, batch, pred, thetas, alpha=1.0, **axis_sweep_kw):
    """demo.py:67-82 down to the tables: ``axis_sweep`` (its keywords pass through), then per angle the ``1 + nc`` one-column grids side
    by side, every cell normalised by its own range -- all T frames composed in one call (``wu.grid.demo_tables``).  Returns
    (T, Hg, Wg, 3) uint8 on the GPU: the input of the encoders and of ``save_demo``."""
    from . import grid
    return grid.demo_tables(batch, axis_sweep(transfer, batch, pred, thetas, alpha, **axis_sweep_kw), out="uint8")


def save_demo(frames_u8, out, encoder=None, png_encoder=None, ext=".jpg", stem="frame", gif_encoder=None):
    """Writes the frames of ``demo_frames``.  ``out`` ending in .gif: the animation of demo.py:86-92 -- ping-pong order ``frames[0],
    frames[1:] + frames[1:-1][::-1]``, ``duration=1000 // T``, ``loop=0``.  With ``gif_encoder`` (a ``wu.gif_enc.GPUGifEncoder``) palette
    and LZW run on the GPU, every distinct frame once, and the finished image blocks are what is fetched; without it Pillow writes the file
    from the frames fetched as raw RGB.  Anything else is a directory: one file ``{stem}{t:04d}{ext}`` per frame through the GPU encoders,
    routed by ``ext`` as ``save_images`` routes.  Returns the path of the GIF, or the list of files."""
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.dtype != torch.uint8:
        raise ValueError(f"save_demo: (T, Hg, Wg, 3) uint8 frames, got {tuple(frames_u8.shape)} {frames_u8.dtype}")
    out = os.fspath(out)
    T = frames_u8.shape[0]
    if out.lower().endswith(".gif"):
        if gif_encoder is not None:
            from .gif_enc import ping_pong
            data = gif_encoder.encode(frames_u8, 1000 // T, 0, ping_pong(T))
            with open(out, "wb") as fh:
                fh.write(data)
            return out
        from PIL import Image
        rgb = frames_u8.cpu().numpy()
        imgs = [Image.fromarray(f).convert("RGB") for f in rgb]
        imgs[0].save(out, save_all=True, append_images=imgs[1:] + imgs[1:-1][::-1], duration=1000 // T, loop=0)
        return out
    os.makedirs(out, exist_ok=True)
    paths = [os.path.join(out, f"{stem}{t:04d}{ext}") for t in range(T)]
    for f in _save_u8_async(frames_u8, paths, encoder, png_encoder):
        f.result()
    return paths


# ---- full-resolution output (wu.guided) ------------------------------------------------------------------------------------------------------
@torch.no_grad()
def transfer_fullres(transfer, photos_u8, sizes, rows, input_size, normalize=True, upsampler=None, shared_encoder=True, graphed=None):
    """The transfer at the PHOTOGRAPH's resolution: ``photos_u8`` (N, Hmax, Wmax, 3) uint8 with per-image ``sizes`` (h, w), as the decoders
    leave a batch.  (1) ``GPUInputPipeline(input_size, train=False)`` makes the network input (N, 3, S, S); (2) the sweep over ``rows`` --
    (R, nc): every image under every row, as ``signal_sweep``; (R, N, nc): every image under its own rows (one row per image, as
    ``transfer_rows``, is (1, N, nc)) --; (3) the low-resolution target is ``normalize_minmax`` of each output, exactly what ``save_images``
    would have written, or ``(out + 1) / 2`` with ``normalize=False``; (4) ``upsampler`` (a ``wu.guided.GuidedUpsampler``; default: one with
    its untuned default r and eps) fits the target to the network input and applies the fit to the photograph.  Returns the padded
    (R, N, Hmax, Wmax, 3) uint8 batch the encoders take with ``sizes``.  ``shared_encoder`` / ``graphed``: see ``signal_sweep`` (rows of
    three dimensions need the shared encoder)."""
    from .guided import GuidedUpsampler
    from .input_pipeline import GPUInputPipeline
    batch = GPUInputPipeline(input_size, train=False)(photos_u8, sizes)
    rows = rows.to(device=batch.device, dtype=torch.float32)
    if rows.dim() == 3:
        if rows.shape[1] != batch.shape[0]:
            raise ValueError(f"transfer_fullres: rows (R, N, nc) for N = {batch.shape[0]} images, got {tuple(rows.shape)}")
        if not shared_encoder:
            raise ValueError("transfer_fullres: rows per image (R, N, nc) go through the shared-encoder sweep")
        out = _sweep(transfer, batch, rows, graphed, None)
    elif rows.dim() == 2:
        out = signal_sweep(transfer, batch, rows, False, graphed, shared_encoder)
    else:
        raise ValueError(f"transfer_fullres: rows (R, nc) or (R, N, nc), got {tuple(rows.shape)}")
    out = out.float()
    low = _normalize_all(out, True) if normalize else (out + 1) / 2
    up = upsampler if upsampler is not None else GuidedUpsampler()
    return up.upsample(batch, low, photos_u8, sizes)


def _decode_files(files, decoder):
    """(photos_u8, sizes) of one batch of files: all .jpg / .jpeg through a ``GPUJpegDecoder``, anything else through ``wu.png.decode_mixed``
    (segmented PNGs on the GPU, the rest by Pillow)."""
    if all(os.fspath(f).lower().endswith((".jpg", ".jpeg")) for f in files):
        if decoder is not None:
            return decoder.decode_batch(files)
        from .jpeg import GPUJpegDecoder
        dec = GPUJpegDecoder()
        try:
            return dec.decode_batch(files)
        finally:
            dec.close()
    from .png import decode_mixed
    return decode_mixed(files)


def _save_padded_async(u8, sizes, paths, encoder, png_encoder):
    """``_save_u8_async`` for a padded batch: (N, Hmax, Wmax, 3) uint8 with per-image (h, w)."""
    ext = os.path.splitext(paths[0])[1].lower()
    if ext in (".jpg", ".jpeg"):
        return [(encoder if encoder is not None else _encoder(u8)).save_batch_async(u8, paths, sizes)]
    if ext == ".png" and png_encoder is not None:
        return [png_encoder.save_batch_async(u8, paths, sizes)]
    rgb = u8.cpu().numpy()
    for i, (h, w) in enumerate(sizes):
        _pillow_save((rgb[i, :h, :w], paths[i]))
    return []


@torch.no_grad()
def fullres_sweep_to_dir(transfer, files, src_labels, class_names, out_dir, input_size=224, ext=".jpg", decoder=None, encoder=None,
                         png_encoder=None, rows=None, row_names=None, normalize=True, upsampler=None, shared_encoder=True, graphed=None):
    """``class_sweep_to_dir`` at the photographs' own sizes, from files to files: ``files`` are decoded on the GPU (``decoder``: a
    ``GPUJpegDecoder`` for an all-JPEG list; other lists go through ``wu.png.decode_mixed``), transferred by ``transfer_fullres`` under every
    class (or under ``rows`` (R, nc) named ``row_names``, default ``row0000``, ...), and written with ``class_sweep_to_dir``'s names,
    ``{class_names[src_labels[j]]}_{stem of files[j]}_{target name}{ext}`` (without the first part when ``src_labels`` is None), each file
    h x w like its source: .jpg / .jpeg by ``encoder`` (default: the shared ``GPUJpegEncoder``), .png by ``png_encoder`` when one is passed,
    any other format by Pillow.  All files exist when this returns; returns the paths, target by target."""
    files = [os.fspath(f) for f in files]
    if src_labels is not None and len(src_labels) != len(files):
        raise ValueError("fullres_sweep_to_dir: one source label per file")
    photos, sizes = _decode_files(files, decoder)
    if rows is None:
        rows = torch.eye(len(class_names), device=photos.device)
        names = list(class_names)
    else:
        names = list(row_names) if row_names is not None else [f"row{r:04d}" for r in range(rows.shape[0])]
        if len(names) != rows.shape[0]:
            raise ValueError("fullres_sweep_to_dir: one name per row")
    out = transfer_fullres(transfer, photos, sizes, rows, input_size, normalize, upsampler, shared_encoder, graphed)
    os.makedirs(out_dir, exist_ok=True)
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    written, pending = [], []
    for i, name in enumerate(names):
        paths = [os.path.join(out_dir, (f"{class_names[int(src_labels[j])]}_" if src_labels is not None else "") + f"{stems[j]}_{name}{ext}")
                 for j in range(len(files))]
        pending += _save_padded_async(out[i], sizes, paths, encoder, png_encoder)
        written += paths
    for f in pending:
        f.result()
    return written
