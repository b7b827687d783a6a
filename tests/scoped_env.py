"""``with Env(RTS_SDP_CONFIG=2): ...`` -- environment knobs of the library for the length of a block, put back after it
(a knob that was unset is unset again).  The library reads its knobs with getenv() at the call or at create."""
import os


class Env(object):
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update({k: str(v) for k, v in self.kw.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
