"""The reference's workflows as functions with a command line each (`python -m geograypher_amd.entrypoints.<name>`)."""

__all__ = ["determine_minimum_overlapping_images", "project_detections"]


def __getattr__(name):   # on first use: `python -m` of an entrypoint must not find its module imported already
    if name == "determine_minimum_overlapping_images":
        from geograypher_amd.entrypoints.annotation_image_selection import determine_minimum_overlapping_images

        return determine_minimum_overlapping_images
    if name == "project_detections":
        import importlib

        return importlib.import_module("geograypher_amd.entrypoints.project_detections").project_detections
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
