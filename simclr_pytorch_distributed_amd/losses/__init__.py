from .barlow import BarlowTwinsLoss, barlow_reference  # noqa: F401
