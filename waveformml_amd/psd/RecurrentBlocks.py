"""Alias module: the reference's ``src.models.RecurrentBlocks`` names (``RecurrentBlock``, ``RecurrentNet``)."""
from .recurrent import RecurrentBlock, RecurrentNet  # noqa: F401
