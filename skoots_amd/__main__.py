"""``python -m skoots_amd --image P --pretrained-checkpoint C [--log 0-4]``: the eval flags of
the reference CLI (skoots/__main__.py:19-46, 78-98), and ``--skeletonize-train-data PATH [--mask-filter .labels]
[--anisotropyXY a] [--anisotropyZ b]`` (skoots/__main__.py:49-68, 101-106), and ``--convert PATH``: eval's zarr stores
and ``.trch`` tensors under PATH -> TIFF stacks, no eval (skoots/__main__.py:70-74, 84, 108-109).  With it every switch of
the reference's main command exists here.  ``--pyramid`` (not in the reference) makes eval also write
``<base>_skoots.ome.zarr``, the multiscale OME-Zarr group of image, instance mask and skeleton.  ``--rescale FX FY FZ``
(not in the reference) resamples the image by those factors before the network and writes the mask on the input's grid.
``--denoise HOW A B C`` (not in the reference) filters the integer image on the device before that: ``HOW`` one of
``median | mean | min | max`` with three integer radii, or ``gauss`` with three sigmas in voxels.  ``--equalize`` (not in
the reference) transforms the grey values of the integer image after that: ``stretch LOW HIGH`` (percentiles), ``clahe TX
TY TZ CLIP`` (contrast-limited adaptive equalisation in tiles), ``match REF.tif`` (the histogram of another image) or
``slices`` (every z-plane matched to the whole stack)."""
import argparse
import glob
import logging
import os


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog="SKOOTS (MI355X)", description="skoots parameters")
    eval_args = parser.add_argument_group("eval arguments")
    eval_args.add_argument("--image", type=str,
                           help="path to image (or a directory of *.tif); required unless --skeletonize-train-data "
                                "or --convert")
    eval_args.add_argument("--pretrained-checkpoint", type=str, help="path to a pretrained skoots model")
    eval_args.add_argument("--use-cached", action="store_true",
                           help="skips model evaluation and loads previously evaluated arrays")
    eval_args.add_argument("--log", type=int, default=3,
                           help="Log Level: 0-Debug, 1-Info, 2-Warning, 3-Error, 4-Critical")
    eval_args.add_argument("--output-huffman", choices=("fixed", "dynamic"), default=None,
                           help="Huffman code of the device deflate encoder that writes the zarr chunks and TIFF pages "
                                "(eval and --convert); default: skoots_amd.lib.eval.OUTPUT_HUFFMAN")
    eval_args.add_argument("--pyramid", action="store_true",
                           help="also writes <base>_skoots.ome.zarr: multiscale pyramids of the image, the instance mask "
                                "and the skeleton as one OME-Zarr group (skoots_amd.utils.pyramid)")
    eval_args.add_argument("--denoise", type=str, nargs=4, default=None, metavar=("HOW", "A", "B", "C"),
                           help="filters the integer image on the device before the network (and before --rescale), mirror "
                                "borders: HOW is median, mean, min or max with three integer radii along x, y and z, or gauss "
                                "with three sigmas in voxels (skoots_amd.lib.morphology.filter_volume)")
    eval_args.add_argument("--equalize", type=str, nargs="+", default=None, metavar="HOW",
                           help="transforms the grey values of the integer image on the device before the network (after "
                                "--denoise, before --rescale): 'stretch LOW HIGH' sends those percentiles to 0 and the maximum, "
                                "'clahe TX TY TZ CLIP' equalises in tiles of that size with the histogram clipped at CLIP times "
                                "its mean, 'match REF.tif' matches the histogram of that image, 'slices' matches every z-plane "
                                "to the whole stack (skoots_amd.lib.morphology.equalize)")
    eval_args.add_argument("--rescale", type=float, nargs=3, default=None, metavar=("FX", "FY", "FZ"),
                           help="output voxels per input voxel along x, y and z: the image is resampled on the device to the "
                                "voxel size the model was trained at, the instance mask is written on the input's own grid "
                                "(skoots_amd.lib.morphology.resample)")
    accessory_args = parser.add_argument_group("scripting arguments")
    accessory_args.add_argument("--skeletonize-train-data",
                                help="calculate skeletons of training data (a label TIFF or a directory of them)")
    accessory_args.add_argument("--mask-filter", default=".labels", help="filter of mask file")
    accessory_args.add_argument("--anisotropyXY", type=float, default=1.0, help="resample factor of x and y")
    accessory_args.add_argument("--anisotropyZ", type=float, default=1.0, help="resample factor of z")
    accessory_args.add_argument("--convert", type=str,
                                help="converts all skoots eval outputs in directory to a tif image")
    return parser


def equalize_option(words) -> dict:
    """``--equalize``'s words as ``eval``'s ``equalize`` dict: ``stretch LOW HIGH``, ``clahe TX TY TZ CLIP``, ``match
    REF.tif`` or ``slices``"""
    from skoots_amd.lib.eval import equalize_arguments
    how, rest = words[0], list(words[1:])
    forms = {"stretch": 2, "clahe": 4, "match": 1, "slices": 0}
    if how not in forms or len(rest) != forms[how]:
        raise ValueError(f"takes 'stretch LOW HIGH', 'clahe TX TY TZ CLIP', 'match REF.tif' or 'slices', got {' '.join(words)!r}")
    if how == "stretch":
        option = {"how": "stretch", "low": float(rest[0]), "high": float(rest[1])}
    elif how == "clahe":
        option = {"how": "equalize", "tile": tuple(int(v) for v in rest[:3]), "clip": float(rest[3])}
    elif how == "match":
        option = {"how": "match", "target": rest[0]}
    else:
        option = {"how": "match", "tile": "slices"}
    equalize_arguments(option)
    return option


def parse_args(argv=None) -> argparse.Namespace:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.denoise is not None:
        from skoots_amd.lib.eval import denoise_arguments
        how, numbers = args.denoise[0], args.denoise[1:]
        try:
            numbers = tuple(float(v) if how == "gauss" else int(v) for v in numbers)
            denoise_arguments((how, numbers))
        except ValueError as e:
            parser.error(f"--denoise: {e}")
        args.denoise = (how, numbers)
    if args.equalize is not None:
        try:
            args.equalize = equalize_option(args.equalize)
        except (ValueError, FileNotFoundError) as e:
            parser.error(f"--equalize: {e}")
    if args.skeletonize_train_data is None and args.convert is None and args.image is None:
        parser.error("the following arguments are required: --image")
    if args.rescale is not None and not all(0 < v < float("inf") for v in args.rescale):
        parser.error("--rescale must be three positive finite numbers")
    if args.rescale is not None and args.pyramid:
        parser.error("--pyramid together with --rescale is not built: run python -m skoots_amd.utils.pyramid on the outputs")
    return args


def main(argv=None):
    args = parse_args(argv)
    levels = [logging.DEBUG, logging.INFO, logging.WARNING, logging.ERROR, logging.CRITICAL]
    logging.basicConfig(level=levels[args.log], format="[%(asctime)s] skoots-eval [%(levelname)s]: %(message)s")
    if args.skeletonize_train_data is not None:
        from skoots_amd.train.generate_skeletons import create_gt_skeletons
        scale = (args.anisotropyXY, args.anisotropyXY, args.anisotropyZ)
        print("skeletonizing...")
        create_gt_skeletons(args.skeletonize_train_data, args.mask_filter, scale)
    if args.convert is not None:
        from skoots_amd.utils.convert_trch_to_tif import convert
        convert(args.convert, huffman=args.output_huffman)
    if args.skeletonize_train_data is not None or args.convert is not None:   # no eval (skoots/__main__.py:84)
        return
    assert args.pretrained_checkpoint is not None, (
        "Cannot evaluate SKOOTS wihtout pretrained model. --pretrained_checkpoint must not be None")
    from skoots_amd.lib.eval import eval as sk_eval
    files = sorted(glob.glob(args.image + "/*.tif")) if os.path.isdir(args.image) else [args.image]
    for f in files:
        extra = {"pyramid": True} if args.pyramid else {}   # the keywords go down only when they are set
        if args.rescale is not None:
            extra["rescale"] = tuple(args.rescale)
        if args.denoise is not None:
            extra["denoise"] = args.denoise
        if args.equalize is not None:
            extra["equalize"] = args.equalize
        sk_eval(f, args.pretrained_checkpoint, used_cached_data=args.use_cached, output_huffman=args.output_huffman,
                **extra)


if __name__ == "__main__":
    main()
