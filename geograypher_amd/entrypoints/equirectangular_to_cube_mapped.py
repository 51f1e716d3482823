"""Chip a folder of equirectangular (360-degree) photos into perspective views on the device.

Mirror of geograypher/entrypoints/equirectangular_to_cube_mapped.py:16-300.  Every photo is uploaded once and all its views are
resampled from the device copy; the next photo is decoded on a host thread meanwhile.  Not carried over: the KMeans choice of
photos by projected camera location (`photogrammetry_cameras_path`; it needs a CRS projection this project does not have) and
the mask-sum plot (`visualize_mask_sum`)."""
import argparse
import typing
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from geograypher_amd.utils.image import perspectives_from_equirectangular

# Camera orientations (fov, yaw, pitch) to sample from each equirectangular image: the six faces of a cube
FYPS = [
    (90 - 0.001, 0, -90),
    (90 - 0.001, 0, 90),
    (90 - 0.001, 0, 0),
    (90 - 0.001, 90, 0),
    (90 - 0.001, 180, 0),
    (90 - 0.001, 270, 0),
]
# Sample this many more pixels than the final resolution before downsampling
OVERSAMPLE_FACTOR = 4
# Order of interpolation
WARP_ORDER = 1
# One quarter of the width of the GoPro MAX2 equirectangular image
OUTPUT_SIZE = (1920, 1920)
IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".tif", ".tiff")


def _imread(path) -> np.ndarray:
    from PIL import Image

    with Image.open(path) as im:
        return np.asarray(im)


def _imwrite(path, array):
    from PIL import Image

    Image.fromarray(array).save(path)


def select_files(input_dir: Path, n_images_to_save: typing.Optional[int], image_extensions=IMAGE_EXTENSIONS,
                 seed: typing.Optional[int] = None) -> list:
    """The photos to chip (entrypoint lines 72-142): every image under `input_dir`, or `n_images_to_save` of every
    (len // n)-th one, drawn without replacement by numpy.random.default_rng(seed)."""
    files = sorted(f for f in Path(input_dir).rglob("*") if f.is_file() and f.suffix.lower() in image_extensions)
    if n_images_to_save is None:
        return files
    stride = max(1, len(files) // n_images_to_save)
    candidates = files[::stride]
    picked = np.random.default_rng(seed).choice(len(candidates), size=n_images_to_save, replace=False)
    return [candidates[i] for i in picked]


def chip_equirectangular_folder(
    input_dir: Path,
    output_dir: Path,
    fyps: typing.List[typing.Tuple[float, float, float]],
    n_images_to_save: typing.Optional[int],
    output_size: typing.Tuple[int, int],
    oversample_factor: int,
    warp_order: int,
    photogrammetry_cameras_path: typing.Optional[Path] = None,
    image_extensions: typing.Sequence[str] = IMAGE_EXTENSIONS,
    seed: typing.Optional[int] = None,
    backend=None,
) -> typing.Optional[np.ndarray]:
    """Write `<stem>_fov{fov}_yaw{yaw}_pitch{pitch}.png` under `output_dir` (keeping the sub-folders of `input_dir`) for every
    chosen photo and every (fov, yaw, pitch) of `fyps`.  Returns the last photo loaded, or None."""
    if photogrammetry_cameras_path is not None:
        raise NotImplementedError(
            "photogrammetry_cameras_path (choosing photos nearest the KMeans centres of the projected camera locations) is not "
            "implemented: it needs a CRS projection.  Leave it None for the sequential subset (reproducible with `seed`).")
    input_dir, output_dir = Path(input_dir), Path(output_dir)
    files_to_save = select_files(input_dir, n_images_to_save, tuple(image_extensions), seed)
    last_img = None
    with ThreadPoolExecutor(max_workers=1) as loader:   # decode the next photo while the device works on this one
        pending = loader.submit(_imread, files_to_save[0]) if files_to_save else None
        for k, f in enumerate(files_to_save):
            last_img = pending.result()
            pending = loader.submit(_imread, files_to_save[k + 1]) if k + 1 < len(files_to_save) else None
            views = perspectives_from_equirectangular(last_img, fyps, output_size=output_size, warp_order=warp_order,
                                                      oversample_factor=oversample_factor, backend=backend)
            for (fov, yaw, pitch), resampled in zip(fyps, views):
                out_path = (output_dir / f.parent.relative_to(input_dir)
                            / f"{f.stem}_fov{int(round(fov))}_yaw{int(round(yaw))}_pitch{int(round(pitch))}.png")
                out_path.parent.mkdir(parents=True, exist_ok=True)
                _imwrite(out_path, resampled.astype(np.uint8))
    return last_img


def visualize_mask_sum(*args, **kwargs):
    raise NotImplementedError("visualize_mask_sum is plotting and is not part of this project; the masks themselves come from "
                              "perspective_from_equirectangular(..., return_mask=True)")


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Chip equirectangular images into perspective views.")
    parser.add_argument("image_dir", type=Path, help="Folder of equirectangular images to process")
    parser.add_argument("output_dir", type=Path, help="Directory the perspective images are written under")
    parser.add_argument("--n-images-to-save", type=int,
                        help="Chip this many original images. If not provided, all images will be saved. (default: None)")
    parser.add_argument("--seed", type=int, help="Seed of the draw behind --n-images-to-save (default: unseeded)")
    parser.add_argument("--oversample-factor", type=int, default=OVERSAMPLE_FACTOR,
                        help=f"Sample this many times more pixels before downsampling (default: {OVERSAMPLE_FACTOR})")
    parser.add_argument("--warp-order", type=int, default=WARP_ORDER,
                        help=f"Interpolation order for warping, 0 or 1 (default: {WARP_ORDER})")
    parser.add_argument("--output-size", type=int, nargs=2, metavar=("HEIGHT", "WIDTH"), default=list(OUTPUT_SIZE),
                        help=f"Output image size in pixels (default: {OUTPUT_SIZE[0]} {OUTPUT_SIZE[1]})")
    parser.add_argument("--visualize-mask-sum-path", type=Path, help="Not implemented (plotting)")
    parser.add_argument("--photogrammetry-cameras-path", help="Not implemented (needs a CRS projection)")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.visualize_mask_sum_path:
        visualize_mask_sum()
    chip_equirectangular_folder(args.image_dir, args.output_dir, FYPS, args.n_images_to_save, tuple(args.output_size),
                                args.oversample_factor, args.warp_order, args.photogrammetry_cameras_path, seed=args.seed)


if __name__ == "__main__":
    main()
