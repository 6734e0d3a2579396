"""MI355X-native DISTS / A-DISTS hot path of kobejean/nerf-qa."""
from ._lib import NqaError  # noqa: F401
from .alias import install_alias, remove_alias  # noqa: F401
from .pair import score_pair  # noqa: F401
from .scoremaps import score_maps  # noqa: F401

__all__ = ["NqaError", "install_alias", "remove_alias", "score_pair", "score_maps"]
