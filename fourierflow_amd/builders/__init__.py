"""Data builders.  Of the reference's ``fourierflow.builders`` the synthetic Navier-Stokes generator and the training set of the
Markov routine are built (``MarkovTrajectoryData``: the pair datasets of ns_markov.py / kolmogorov.py drawn on the device from
whole trajectories); the other dataset classes slice files, and the training commands read ``.npz`` files directly
(fourierflow_amd/cli.py)."""
from .markov_data import MarkovTrajectoryData  # noqa: F401
from .synthetic import Force, GaussianRF, random_force, solve_navier_stokes_2d  # noqa: F401
