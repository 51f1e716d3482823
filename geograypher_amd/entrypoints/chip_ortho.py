"""Cut an orthomosaic into square chips for inference.

Mirror of geograypher/entrypoints/chip_ortho.py: the reference's positional arguments and flags.  All arguments go to
`geograypher_amd.predictors.ortho_segmentor.write_chips`, which writes imagery only: --label-vector-file is refused there."""
import argparse
import json
from pathlib import Path

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
    args = parser.parse_args(argv)
    if args.label_remap is not None:   # (the reference parses it unconditionally and fails without the flag)
        args.label_remap = json.loads(args.label_remap)
    return args


def main(argv=None):
    write_chips(**vars(parse_args(argv)))


if __name__ == "__main__":
    main()
