from geograypher_amd.predictors.segmentor import Segmentor
from geograypher_amd.predictors.derived_segmentors import (
    ArrayLabelSegmentor,
    ImageIDSegmentor,
    LookUpSegmentor,
    RegionDetectionSegmentor,
    TabularRectangleSegmentor,
)

__all__ = ["Segmentor", "LookUpSegmentor", "ArrayLabelSegmentor", "ImageIDSegmentor", "TabularRectangleSegmentor",
           "RegionDetectionSegmentor"]
