"""Merge the predictions made on the chips of an orthomosaic into one georeferenced class raster, on the device.

Mirror of geograypher/entrypoints/assemble_ortho_predictions.py: the reference's positional arguments and flags, and
--count-dtype, which the reference leaves to callers of the function.  All arguments go to
`geograypher_amd.predictors.ortho_segmentor.assemble_tiled_predictions`."""
import argparse
from inspect import signature
from pathlib import Path

import numpy as np

from geograypher_amd.predictors.ortho_segmentor import assemble_tiled_predictions

COUNT_DTYPES = {"uint8": np.uint8, "uint16": np.uint16, "float": float}


def parse_args(argv=None):
    params = signature(assemble_tiled_predictions).parameters
    parser = argparse.ArgumentParser(formatter_class=argparse.RawDescriptionHelpFormatter,
                                     description=__doc__ + "\n\n" + assemble_tiled_predictions.__doc__)
    parser.add_argument("raster_file", type=Path)
    parser.add_argument("pred_folder", type=Path)
    parser.add_argument("class_savefile", type=Path)
    parser.add_argument("num_classes", type=int)
    parser.add_argument("--counts-savefile", type=Path)
    parser.add_argument("--downweight-edge-frac", type=float, default=params["downweight_edge_frac"].default)
    parser.add_argument("--nodataval", type=int, default=params["nodataval"].default)
    parser.add_argument("--max-overlapping-tiles", type=int, default=params["max_overlapping_tiles"].default)
    parser.add_argument("--count-dtype", choices=sorted(COUNT_DTYPES), default="uint8")
    args = parser.parse_args(argv)
    args.count_dtype = COUNT_DTYPES[args.count_dtype]
    return args


def main(argv=None):
    assemble_tiled_predictions(**vars(parse_args(argv)))


if __name__ == "__main__":
    main()
