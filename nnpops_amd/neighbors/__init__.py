"""Neighbour search (reference src/pytorch/neighbors/__init__.py)."""
from .getNeighborPairs import getNeighborPairs  # noqa: F401
from .getNeighborPairsFrames import frame_table, getNeighborPairsFrames  # noqa: F401
