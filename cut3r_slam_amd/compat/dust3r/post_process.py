from src.dust3r.post_process import *  # noqa: F401,F403
from src.dust3r.post_process import __all__  # noqa: F401
