"""drop-in alias of multimae_amd.output_adapter_utils (same public names as the reference's multimae/output_adapter_utils.py)"""
from multimae_amd.output_adapter_utils import *  # noqa: F401,F403
from multimae_amd import output_adapter_utils as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith('__')})
