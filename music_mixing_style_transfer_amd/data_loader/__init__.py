from .data_loader import (Collate_Variable_Length_Segments, MUSDB_Dataset_Mixing_Manipulated_FXencoder,  # noqa: F401
                          MUSDB_Dataset_Mixing_Manipulated_Style_Transfer, Song_Dataset_Inference)
from .loader_utils import (load_wav_length, SlicedWavWriter, StemBank, batch_finish, gather_pcm, get_total_audio_length,  # noqa: F401
                           load_wav_device, load_wav_segment, pcm16_device, save_wav_pcm16)
