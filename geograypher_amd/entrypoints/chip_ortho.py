"""Cut an orthomosaic into square chips for inference, or with --label-vector-file into image chips and label chips for training.

Mirror of geograypher/entrypoints/chip_ortho.py: the reference's positional arguments and flags, and --ROI-file and
--background-ind of its `write_chips`.  All arguments go to `geograypher_amd.predictors.ortho_segmentor.write_chips`; the labels
are burned on the device."""
import argparse
import json
from pathlib import Path

from geograypher_amd.constants import NULL_TEXTURE_INT_VALUE
from geograypher_amd.predictors.ortho_segmentor import write_chips


def parse_args(argv=None):
    parser = argparse.ArgumentParser(formatter_class=argparse.RawDescriptionHelpFormatter, description=__doc__ + "\n\n" + write_chips.__doc__)
    parser.add_argument("raster_file", type=Path)
    parser.add_argument("output_folder", type=Path)
    parser.add_argument("chip_size", type=int)
    parser.add_argument("chip_stride", type=int)
    parser.add_argument("--label-vector-file", help="Path to vector label file.", type=Path)
    parser.add_argument("--label-column", type=str)
    parser.add_argument("--label-remap", type=str,
                        help="Provide this argument as a json-formatted string. For example '{\"name 1\": 0, \"name 2\": 1}'")
    parser.add_argument("--write-empty-tiles", action="store_true")
    parser.add_argument("--ROI-file", dest="ROI_file", type=Path, help="Write only the chips that meet this region (.geojson).")
    parser.add_argument("--background-ind", type=int, default=NULL_TEXTURE_INT_VALUE, help="The label of pixels no polygon holds.")
    args = parser.parse_args(argv)
    if args.label_remap is not None:   # (the reference parses it unconditionally and fails without the flag)
        args.label_remap = json.loads(args.label_remap)
    return args


def main(argv=None):
    write_chips(**vars(parse_args(argv)))


if __name__ == "__main__":
    main()
