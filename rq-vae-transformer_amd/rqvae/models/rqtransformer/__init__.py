"""rqvae/models/rqtransformer/__init__.py of the reference."""
from .transformers import RQTransformer, SampleLogProbs


def get_rqtransformer(config):
    return RQTransformer(config)
