"""Data builders.  Of the reference's ``fourierflow.builders`` only the synthetic Navier-Stokes generator is built: the dataset
classes slice files, and the training commands read ``.npz`` files directly (fourierflow_amd/cli.py)."""
from .synthetic import Force, GaussianRF, random_force, solve_navier_stokes_2d  # noqa: F401
