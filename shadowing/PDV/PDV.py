"""`shadowing.PDV.PDV` import path of the reference, served by shadowing_amd.pdv."""
from shadowing_amd.pdv import *  # noqa: F401,F403
from shadowing_amd.pdv import AutoregressiveLinearPredictor, PDVModel, PDVModelDiscrete  # noqa: F401
