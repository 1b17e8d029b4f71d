"""`shadowing.PDV` import path of the reference (the path-dependent volatility model), served by shadowing_amd.pdv."""
from shadowing_amd.pdv import *  # noqa: F401,F403
