"""MI355X-native PointNet2 hot path of IGNF/StrataNet2-Vegetation-Coverage-Maps.

Mirror of the reference's `model/` package for that path:
    from stratanet2_vegetation_coverage_maps_amd import PointNet2, project_to_plotwise_coverages, project_to_2d_rasters
The HIP library (csrc/libstrata_hip.so) is loaded on first use and is mandatory: there is no CPU fallback.
"""
from .evaluation import evaluate, evaluate_table, plot_losses, plot_losses_torch  # noqa: F401
from .hip_ops import subsample, subsample_form  # noqa: F401
from .inference import AtlasReport, MosaicAtlas, PointScoreResult, PointScores  # noqa: F401
from .parcel import (ParcelClouds, ParcelCut, ParcelPlots, ParcelSet, cut_parcels, parcel_plot_centers, polygon_keep,  # noqa: F401
                     predict_parcel_cloud, predict_parcels, prepare_parcel, prepare_parcels)
from .point_net2 import PointNet2  # noqa: F401
from .project_to_2d import (project_batch_to_2d_rasters, project_to_2d_rasters,  # noqa: F401
                            project_to_plotwise_coverages)
from .train_data import EpochFeeder, ResidentPlots  # noqa: F401
from .pseudo_label import label_plots, pretrain_split, pseudo_label_parcel  # noqa: F401
from .cross_validation import CrossValReport, cross_validate, indicators, kfold_indices  # noqa: F401
from . import las  # noqa: F401
from .las import LasHeader, load_las, load_parcel_clouds, load_parcels, load_plot  # noqa: F401
from . import geotiff  # noqa: F401
from . import ortho  # noqa: F401
from .ortho import ColorizeResult, OrthoImage, OrthoSet  # noqa: F401
from . import shp  # noqa: F401

__all__ = ["PointNet2", "project_to_plotwise_coverages", "project_to_2d_rasters", "project_batch_to_2d_rasters", "ParcelPlots",
           "parcel_plot_centers", "polygon_keep", "prepare_parcel", "predict_parcel_cloud", "subsample", "subsample_form",
           "evaluate", "plot_losses", "plot_losses_torch", "ResidentPlots", "EpochFeeder", "label_plots",
           "pseudo_label_parcel", "pretrain_split", "ParcelSet", "ParcelClouds", "prepare_parcels", "predict_parcels", "MosaicAtlas", "AtlasReport",
           "evaluate_table", "kfold_indices", "indicators", "CrossValReport", "cross_validate", "las", "LasHeader",
           "load_las", "load_plot", "load_parcel_clouds", "ParcelCut", "cut_parcels", "load_parcels", "geotiff", "ortho",
           "OrthoImage", "OrthoSet", "ColorizeResult", "shp"]
