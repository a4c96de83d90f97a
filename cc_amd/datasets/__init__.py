"""Training data (the reference's datasets/sequence_folders.py) and its device-resident form.

`crawl` / `SequenceFolder`: the reference's folder format and sample order on the host.  `FrameStore`: every distinct frame decoded
once and kept in HBM as uint8; `DeviceSequenceLoader`: batches built on the device from frame indices, in the form
`CCTrainer.step` takes."""
from .sequence_folders import SequenceFolder, crawl, load_as_float, load_as_uint8
from .frame_store import FrameStore
from .loader import DeviceSequenceLoader

__all__ = ["SequenceFolder", "crawl", "load_as_float", "load_as_uint8", "FrameStore", "DeviceSequenceLoader"]
