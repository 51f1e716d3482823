"""tests/golden/make_golden_equirect.py -- golden vectors for the 360-degree (equirectangular) input path.

Two stages, because no single interpreter of this container has every dependency of the reference:

  stage "views" (/opt/conda/bin/python3.9, which has scikit-image 0.18.3 and scipy 1.7.1; piexif stubbed): the REAL
      utils.image.perspective_from_equirectangular (utils/image.py:129-267) and rotate_by_roll_pitch_yaw (image.py:29-69) on
      small seeded sources.
          PYTHONPATH=/root/reference /opt/conda/bin/python3.9 tests/golden/make_golden_equirect.py views
  stage "rig" (python3.10 + MagicMock stubs, see make_golden.py): the REAL
      cameras.rig_cameras.create_rig_cameras_from_equirectangular (rig_cameras.py:9-105) on tests/golden/metashape_camera.xml.
          PYTHONPATH=/root/reference python tests/golden/make_golden_equirect.py rig

Output: tests/golden/reference_equirect.npz (inputs included).  Sources are at most 128 x 256.
"""
import sys
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np

HERE = Path(__file__).resolve().parent
OUT = HERE / "reference_equirect.npz"

# name -> (source, fov, yaw, pitch, roll, output_size, oversample_factor, warp_order)
VIEWS = {
    "down": (89.999, 0, -90, 0, (24, 24), 4, 1),      # three faces of the entrypoint's rig (FYPS)
    "right": (89.999, 90, 0, 0, (24, 24), 4, 1),
    "back": (89.999, 180, 0, 0, (24, 24), 4, 1),      # straddles the wrap-around column
    "rolled": (70.0, 33.0, 21.0, 17.0, (20, 31), 2, 1),
    "os1": (60.0, 200.0, -35.0, 0, (37, 41), 1, 1),
    "nearest": (75.0, 300.0, 40.0, 10.0, (22, 26), 2, 0),
}
SOURCES = ("u8", "sat", "f64")
ROTATIONS = [(0, 0, 0), (0, -90, 0), (0, 0, 90), (0, 0, 180), (17.0, 21.0, 33.0), (30, 45, 270), (180, 90, 45), (-12.5, 7.25, 301.0)]
RIG_ORIENTATIONS = [
    {"roll_deg": 0, "pitch_deg": -90, "yaw_deg": 0},
    {"roll_deg": 0, "pitch_deg": 0, "yaw_deg": 90},
    {"roll_deg": 17.0, "pitch_deg": 21.0, "yaw_deg": 33.0},
]
RIG_FORMAT = "_yaw{yaw_deg:.0f}_pitch{pitch_deg:.0f}_roll{roll_deg:.0f}"
RIG_CAMERA = {"f": 960.0, "cx": 0.0, "cy": 0.0, "image_width": 1920, "image_height": 1920}


def make_sources():
    rng = np.random.default_rng(360)
    u8 = rng.integers(0, 256, size=(96, 192, 3), dtype=np.uint8)
    sat = u8.copy()
    sat[:40] = 255
    # unit-scale values, some negative (vmin < 0 moves the normalised fill): the numpy of the two interpreters differs by an ulp
    # in arctan2 / arcsin, 1.4e-14 px at these sizes, which a texel step of 1 turns into 1e-14 of value
    f64 = rng.random((64, 128, 2)) - 0.25
    return {"u8": u8, "sat": sat, "f64": f64}


def stage_views():
    sys.modules["piexif"] = MagicMock()
    sys.path.insert(0, "/root/reference")
    from geograypher.utils.image import perspective_from_equirectangular, rotate_by_roll_pitch_yaw

    out = {"src_" + k: v for k, v in make_sources().items()}
    for name, (fov, yaw, pitch, roll, size, os_, order) in VIEWS.items():
        out["view_" + name] = np.array([fov, yaw, pitch, roll, size[0], size[1], os_, order], dtype=np.float64)
        for s in SOURCES:
            img, mask = perspective_from_equirectangular(out["src_" + s], fov, output_size=size, yaw_deg=yaw, pitch_deg=pitch,
                                                         roll_deg=roll, warp_order=order, oversample_factor=os_,
                                                         return_mask=True)
            out[f"out_{s}_{name}"] = img
            out[f"mask_{s}_{name}"] = mask
    out["rpy"] = np.array(ROTATIONS, dtype=np.float64)
    out["rot3"] = np.stack([rotate_by_roll_pitch_yaw(*r) for r in ROTATIONS])
    out["rot4"] = np.stack([rotate_by_roll_pitch_yaw(*r, return_4x4=True) for r in ROTATIONS])
    np.savez_compressed(OUT, **out)
    print("views written:", len(out), "arrays")


def stage_rig():
    sys.path.insert(0, str(HERE))
    import make_golden  # the stub finder

    sys.meta_path.insert(0, make_golden._Finder())
    sys.path.insert(0, make_golden.REFERENCE)
    import tempfile

    import pyproj

    pyproj.Transformer.from_crs.return_value.transform.side_effect = lambda xx, yy, zz: (0 * xx, 0 * xx, 0 * xx)
    from geograypher.cameras.rig_cameras import create_rig_cameras_from_equirectangular

    with np.load(OUT) as d:
        out = {k: d[k] for k in d.files}
    with tempfile.TemporaryDirectory() as tmp:
        p = Path(tmp, "camera.xml")
        p.write_text((HERE / "metashape_camera.xml").read_text())
        rig = create_rig_cameras_from_equirectangular(
            camera_file=p, original_images="/home/user/image_sets", perspective_images="/data/perspective",
            rig_camera=RIG_CAMERA, rig_orientations=RIG_ORIENTATIONS, perspective_filename_format_str=RIG_FORMAT)
    out["rig_transforms"] = np.stack([c.cam_to_world_transform for c in rig.cameras])
    out["rig_filenames"] = np.array([str(c.image_filename) for c in rig.cameras])
    out["rig_local_to_epsg_4978"] = np.asarray(rig.get_local_to_epsg_4978_transform(), dtype=np.float64)
    np.savez_compressed(OUT, **out)
    print("rig written:", len(rig.cameras), "cameras")


if __name__ == "__main__":
    {"views": stage_views, "rig": stage_rig}[sys.argv[1]]()
