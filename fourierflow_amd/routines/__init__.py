from .grid_2d_markov import Grid2DMarkovExperiment  # noqa: F401
from .grid_2d_rollout import Grid2DRolloutExperiment  # noqa: F401
from .structured_mesh import StructuredMeshExperiment  # noqa: F401
from .point_cloud import PointCloudExperiment  # noqa: F401

KINDS = {"Grid2DMarkovExperiment": "markov", "Grid2DRolloutExperiment": "rollout", "StructuredMeshExperiment": "mesh",
         "PointCloudExperiment": "pointcloud"}


def routine_kind(routine) -> str:
    """The short name of the routine's class: what the commands and the batch sources dispatch on."""
    return KINDS[type(routine).__name__]
