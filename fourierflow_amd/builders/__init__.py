"""Data builders.  Of the reference's ``fourierflow.builders`` these are built: the synthetic Navier-Stokes generator; the
training set of the Markov routine (``MarkovTrajectoryData``: the pair datasets of ns_markov.py / kolmogorov.py drawn on the
device from whole trajectories); and the dataset builders of the mesh and point-cloud experiments (``StructuredMesh2DBuilder``,
``PlasticityBuilder``, ``ElasticityBuilder``: the datasets' own files, split as the reference splits them, held on the device as
``DeviceSampleData``), of the torus_li experiments (``NSMarkovBuilder``, ``NSZongyiBuilder``: builders/ns_data.py) and of the
contextual torus_vis / torus_vis_force experiments (``NSContextualBuilder``: builders/ns_contextual.py) and of the Kolmogorov-flow
torus_kochkov experiments (``KolmogorovBuilder`` with its two datasets and the multi-resolution training set
``KolmogorovMultiResolutionDataset`` / ``MultiResolutionMarkovData``: builders/kolmogorov.py), whose files the Kolmogorov-flow generator writes
(``generate_kolmogorov``, ``KolmogorovStepper``, ``initial_vorticity``: builders/kolmogorov_flow.py).  Without a builder the training commands read ``.npz`` files directly (fourierflow_amd/cli.py)."""
from .kolmogorov import (KolmogorovBuilder, KolmogorovJAXDataset, KolmogorovJAXTrajectoryDataset,  # noqa: F401
                         KolmogorovMultiResolutionDataset, KolmogorovMultiTorchDataset, KolmogorovTorchDataset,
                         KolmogorovTrajectoryDataset)
from .kolmogorov_flow import (KolmogorovPlan, KolmogorovStepper, generate_kolmogorov, initial_vorticity,  # noqa: F401
                              plan_kolmogorov, stable_time_step)
from .markov_data import MarkovTrajectoryData, MultiResolutionMarkovData  # noqa: F401
from .mesh_data import ElasticityBuilder, PlasticityBuilder, StructuredMesh2DBuilder  # noqa: F401
from .ns_contextual import NSContextualBuilder  # noqa: F401
from .ns_data import NSMarkovBuilder, NSZongyiBuilder  # noqa: F401
from .sample_data import DeviceSampleData  # noqa: F401
from .synthetic import Force, GaussianRF, random_force, random_force_amplitudes, solve_navier_stokes_2d, solve_navier_stokes_2d_varying_force  # noqa: F401
