"""Training and validation data (the reference's datasets/sequence_folders.py and validation_folders.py) and
their device-resident forms.

`crawl` / `SequenceFolder`: the reference's folder format and sample order on the host.  `FrameStore`: every distinct frame decoded
once and kept in HBM as uint8; `DeviceSequenceLoader`: batches built on the device from frame indices, in the form
`CCTrainer.step` takes.  `ValidationSet`: the depth validation folder on the host; `DepthValStore` / `DeviceDepthValLoader` and
`FlowValStore` / `DeviceFlowValLoader`: the two validation sets in HBM (validation.py).  `prepare` (a module: `KittiRaw`,
`Cityscapes`, `prepare()`): from a KITTI raw or Cityscapes download to these folders and stores (data/prepare_train_data.py)."""
from .sequence_folders import SequenceFolder, crawl, load_as_float, load_as_uint8
from .frame_store import FrameStore
from .loader import DeviceSequenceLoader
from .validation import ValidationSet, crawl_validation, DepthValStore, DeviceDepthValLoader, FlowValStore, DeviceFlowValLoader

__all__ = ["SequenceFolder", "crawl", "load_as_float", "load_as_uint8", "FrameStore", "DeviceSequenceLoader",
           "ValidationSet", "crawl_validation", "DepthValStore", "DeviceDepthValLoader", "FlowValStore", "DeviceFlowValLoader"]
