"""Model classes (mirror of reference src/models)."""
from .tsvgp import base_SVGP, t_SVGP
from .tsvgp_sites import t_SVGP_sites
from .tsvgp_white import t_SVGP_white
from .tvgp import t_VGP

__all__ = ["base_SVGP", "t_SVGP", "t_SVGP_white", "t_SVGP_sites", "t_VGP"]
