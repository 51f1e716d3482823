"""The reference's utils/visualization.py without pyvista and matplotlib: the colour choice of a label table, the three-panel
composite of a photo and a label image on the device (`gr_composite_labels`) and the folder walk that
writes one composite per rendered label.  The colour tables are `utils.colormaps`."""
import json
import logging
import typing
from pathlib import Path

import numpy as np

from geograypher_amd.utils import colormaps

PATH_TYPE = typing.Union[str, Path]


def get_vis_options_from_IDs_to_labels(IDs_to_labels: typing.Union[None, dict], cmap_continous: str = "viridis",
                                       cmap_10_classes: str = "tab10", cmap_20_classes: str = "tab20",
                                       cmap_many_classes: str = "viridis") -> dict:
    """The reference's choice (utils/visualization.py:55-110): no table -> continuous; a largest ID below 10 -> tab10, below 20
    -> tab20, both discrete; more classes -> the continuous map.  {"cmap", "vmin", "vmax", "discrete"}."""
    if IDs_to_labels is None:
        return {"cmap": cmap_continous, "vmin": None, "vmax": None, "discrete": False}
    max_ID = np.max(list(IDs_to_labels.keys()))
    if max_ID < 10:
        return {"cmap": cmap_10_classes, "vmin": -0.5, "vmax": 9.5, "discrete": True}
    if max_ID < 20:
        return {"cmap": cmap_20_classes, "vmin": -0.5, "vmax": 19.5, "discrete": True}
    return {"cmap": cmap_many_classes, "vmin": None, "vmax": None, "discrete": False}


def _default_backend():
    from geograypher_amd._hip import HipRaster

    return HipRaster()


def composite_scalars(label_t, discrete: bool):
    """(shift, scale) of a continuous one-channel label tensor, as the reference takes them (V11): shift = nanmin of the values,
    scale = the largest shifted value among the pixels that are neither 0 nor non-finite (1.0 where there is none), a uint8
    label counting as value / 255.  torch selects the smallest and the largest VALUE on the label's device -- the shifted maximum
    is the shifted largest value, a rounded difference being monotonic --, the two roundings are Python's, on the host."""
    import torch

    if discrete or label_t.ndim == 3:
        return 0.0, 1.0
    if label_t.dtype == torch.uint8:
        lowest = float(label_t.min().item()) / 255
        nonzero = label_t[label_t != 0]
        return lowest, (float(nonzero.max().item()) / 255 - lowest) if nonzero.numel() else 1.0
    x = label_t.to(torch.float64)
    numbers = x[~torch.isnan(x)]
    shift = float(numbers.min().item()) if numbers.numel() else float("nan")
    valid = x[torch.isfinite(x) & (x != 0)]
    return shift, (float(valid.max().item()) - shift) if valid.numel() else 1.0


def create_composite(RGB_image, label_image, label_blending_weight: float = 0.5, IDs_to_labels: typing.Union[None, dict] = None,
                     grayscale_RGB_overlay: bool = True, backend=None):
    """The reference's three-panel composite (utils/visualization.py:113-193) on the device: RGB_image (h, w, 3) uint8 or
    float in [0, 1]; label_image (h, w) [or (h, w, 1)] class IDs or scalars, coloured as `get_vis_options_from_IDs_to_labels`
    says, or (h, w, 3) colours -> (h, 3 w, 3) uint8 [label colours | photo | overlay]: a numpy array for numpy inputs, a tensor
    on the backend's device where either input is a tensor.  ValueError for a uint8 colour label with a discrete table (the
    reference's bytes wrap around there)."""
    import torch

    if backend is None:
        backend = _default_backend()
    if RGB_image.ndim != 3 or RGB_image.shape[2] != 3:
        raise ValueError("Invalid RGB error")
    as_tensor = isinstance(RGB_image, torch.Tensor) or isinstance(label_image, torch.Tensor)
    options = get_vis_options_from_IDs_to_labels(IDs_to_labels)
    if not (label_image.ndim == 3 and label_image.shape[2] == 3):
        label_image = label_image.squeeze() if label_image.ndim > 2 else label_image
        if label_image.ndim != 2:
            raise ValueError(f"label_image must be (h, w), (h, w, 1) or (h, w, 3), got {tuple(label_image.shape)}")
    elif options["discrete"] and str(label_image.dtype).endswith("uint8"):
        raise ValueError("create_composite: a uint8 colour label with discrete IDs_to_labels is not supported")

    def on_device(a):
        dtype = torch.uint8 if str(a.dtype).endswith("uint8") else torch.float64
        return backend._dev(a, dtype)

    photo_t, label_t = on_device(RGB_image), on_device(label_image)
    shift, scale = composite_scalars(label_t, options["discrete"])
    out = backend.composite_labels(photo_t, label_t, colormaps.table(options["cmap"]), discrete=options["discrete"], shift=shift,
                                   scale=scale, weight=float(label_blending_weight), grey_overlay=bool(grayscale_RGB_overlay))
    return out if as_tensor else out.cpu().numpy()


def read_img_npy(filename: PATH_TYPE) -> np.ndarray:
    """A label file: .npy through numpy, everything else (.png, .tif) through PIL."""
    from PIL import Image

    filename = Path(filename)
    if filename.suffix.lower() == ".npy":
        return np.load(filename)
    with Image.open(filename) as image:
        return np.asarray(image)


def show_segmentation_labels(label_folder: PATH_TYPE, image_folder: PATH_TYPE, savefolder: typing.Union[None, PATH_TYPE] = None,
                             num_show: int = 10, label_suffix: str = ".png", image_suffix: str = ".JPG",
                             IDs_to_labels: typing.Optional[dict] = None, seed: typing.Optional[int] = None, backend=None) -> list:
    """One composite per label file under `label_folder` (any of .png, .tif, .npy through `label_suffix`) and the image of the
    same relative path and `image_suffix` under `image_folder`, written as `savefolder/rendered_label_<i>.png` -- the
    reference's call (utils/visualization.py:208-274) with three differences: the files are taken in sorted order and shuffled
    only with a `seed`; without `savefolder` it raises (there is no window to show them in); labels are read from .tif, .png and
    .npy.  IDs_to_labels defaults to `label_folder/IDs_to_labels.json`.  -> the files written."""
    from PIL import Image

    if savefolder is None:
        raise NotImplementedError("show_segmentation_labels: there is no window to show composites in; give a savefolder")
    rendered_files = sorted(Path(label_folder).rglob("*" + label_suffix))
    if seed is not None:
        np.random.default_rng(seed).shuffle(rendered_files)
    Path(savefolder).mkdir(parents=True, exist_ok=True)
    table_file = Path(label_folder, "IDs_to_labels.json")
    if IDs_to_labels is None and table_file.exists():
        IDs_to_labels = {int(k): v for k, v in json.loads(table_file.read_text()).items()}
    if backend is None and rendered_files:
        backend = _default_backend()
    written = []
    for i, rendered_file in enumerate(rendered_files[:num_show]):
        image_file = Path(image_folder, rendered_file.relative_to(label_folder)).with_suffix(image_suffix)
        with Image.open(image_file) as image:
            photo = np.asarray(image.convert("RGB"))
        composite = create_composite(photo, read_img_npy(rendered_file), IDs_to_labels=IDs_to_labels, backend=backend)
        output_file = Path(savefolder, f"rendered_label_{i:03}.png")
        Image.fromarray(composite).save(output_file)
        written.append(output_file)
    logging.getLogger(__name__).info("wrote %d composites to %s", len(written), savefolder)
    return written
