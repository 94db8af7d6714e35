"""toric-rl-decoder_amd: MI355X-native batched toric-code RL environment.

The env hot path of Lindeby/toric-RL-decoder (EnvSet / gym_ToricCode step loop,
generatePerspective, transitions, epsilon-greedy selection) as hand-written HIP kernels
for gfx950 behind a C-ABI (include/toricenv.h), with the reference's Python surface on top.
Import it as ``toric_rl_decoder_amd`` (the directory name has a hyphen).
"""
from ._lib import ToricEnvError, build, load, LIB_PATH
from .stackbuf import alloc_stack, alloc_chunked, configured_xcd_bias, set_xcd_bias
from .transition import TransitionBlock, generateTransitionParallel, to_structured, transition_dtype
from .envset import EnvSet, ToricEnv, generatePerspectiveBatch, make, SUPPORTED_SIZES
from .policy import (NN_11, NN_8, NN_17, NNWideForward, NNWideGrad, ResNet18, ResNet34, ResNetForward, NN11Forward, NN11Grad, NN11Optimizer, learnerStep, evaluate, learnerTargets, predictMaxOptimized, seed_select, segment_max, selectActionBatch, td_target,
                     selectActionEnvSet, _selectActionBatch_prime, prediction_smart,  # noqa: F401
                     generateNPlusQRandomErrors, generateNRandomErrors, generateRandomError)
from .actor import ExploreLoop, computePrioritiesParallel, run_actor
from .replay import PrioritizedReplayMemory

# every public name imported above
__all__ = ["ToricEnvError", "build", "load", "LIB_PATH", "alloc_stack", "alloc_chunked", "configured_xcd_bias", "set_xcd_bias",
           "TransitionBlock", "generateTransitionParallel", "to_structured", "transition_dtype", "EnvSet", "ToricEnv",
           "generatePerspectiveBatch", "make", "SUPPORTED_SIZES", "NN_11", "evaluate", "predictMaxOptimized", "seed_select",
           "segment_max", "selectActionBatch", "selectActionEnvSet", "prediction_smart", "generateNPlusQRandomErrors",
           "generateNRandomErrors", "generateRandomError", "ExploreLoop", "computePrioritiesParallel", "run_actor",
           "PrioritizedReplayMemory", "learnerTargets", "td_target", "NN11Forward",
           "NN11Grad", "learnerStep", "NN11Optimizer", "NN_8", "NN_17", "NNWideForward", "NNWideGrad",
           "ResNet18", "ResNet34", "ResNetForward"]
