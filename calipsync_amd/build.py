"""Build libcasync_hip.so (gfx950) in-tree with hipcc.  No torch extension machinery: the
library is a plain C-ABI shared object loaded with ctypes (calipsync_amd/_lib.py)."""
from __future__ import annotations

import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
OBJ_DIR = os.path.join(LIB_DIR, "obj")
LIB_PATH = os.path.join(LIB_DIR, "libcasync_hip.so")
# Kernels of the bf16 HuBERT handle: compiled to their own object directory (tests/kernel_ledger_hb16.py is their ledger;
# tests/kernel_ledger.py stays the ledger of lib/obj/) and linked into the same library.
OBJ_DIR_HB16 = os.path.join(LIB_DIR, "obj_hb16")
SOURCES_HB16 = ["hubert_bf16.hip"]
# Kernels of the PFLD landmark handle (tests/kernel_ledger_lmk.py is their ledger), the same way.
OBJ_DIR_LMK = os.path.join(LIB_DIR, "obj_lmk")
SOURCES_LMK = ["landmark.hip"]
# Kernels of the S3FD face-detector handle (tests/kernel_ledger_det.py is their ledger): a fourth object directory.  Its
# source is an entry of SOURCES (the list is_stale() and source_hash() walk); SOURCES_DET names which entries compile there.
OBJ_DIR_DET = os.path.join(LIB_DIR, "obj_det")
SOURCES_DET = ["facedet.hip"]
# Kernels of the bf16 precision of the S3FD handle (tests/kernel_ledger_det16.py is their ledger): a fifth object directory, its
# source an entry of SOURCES in the same way.
OBJ_DIR_DET16 = os.path.join(LIB_DIR, "obj_det16")
SOURCES_DET16 = ["facedet_bf16.hip"]
# Kernels of the face pipeline's pixel and row work between the two networks (tests/kernel_ledger_face.py is their ledger): a
# sixth object directory, its source an entry of SOURCES in the same way.
OBJ_DIR_FACE = os.path.join(LIB_DIR, "obj_face")
SOURCES_FACE = ["face_ops.hip"]
# The kernel of S3FD's two NMS passes (tests/kernel_ledger_nms.py is its ledger): a seventh object directory, its source an entry
# of SOURCES in the same way.
OBJ_DIR_NMS = os.path.join(LIB_DIR, "obj_nms")
SOURCES_NMS = ["face_nms.hip"]
# The two byte-move kernels of a clip resident on the device (tests/kernel_ledger_clip.py is their ledger): an eighth object
# directory, its source an entry of SOURCES in the same way.
OBJ_DIR_CLIP = os.path.join(LIB_DIR, "obj_clip")
SOURCES_CLIP = ["clip_ops.hip"]
# The baseline JPEG encoder of finished frames (tests/kernel_ledger_jpeg.py is its ledger): a ninth object directory, its source an
# entry of SOURCES in the same way.
OBJ_DIR_JPEG = os.path.join(LIB_DIR, "obj_jpeg")
SOURCES_JPEG = ["jpeg_enc.hip"]
# Its 4:2:0 sibling (tests/kernel_ledger_jpeg420.py is its ledger): a tenth object directory, its source an entry of SOURCES in
# the same way.  What the two encoders share is csrc/jpeg_enc_common.h (an entry of HEADERS), in each object's own anonymous namespace.
OBJ_DIR_JPEG420 = os.path.join(LIB_DIR, "obj_jpeg420")
SOURCES_JPEG420 = ["jpeg_enc420.hip"]
# The baseline JPEG decoder (tests/kernel_ledger_jpegdec.py is its ledger): an eleventh object directory, its source an entry of
# SOURCES in the same way.  It shares no code with the encoders (their jpeg_enc_common.h is not its header).
OBJ_DIR_JPEGDEC = os.path.join(LIB_DIR, "obj_jpegdec")
SOURCES_JPEGDEC = ["jpeg_dec.hip"]
# The kernels of the SyncNet_color handle (tests/kernel_ledger_sync.py is their ledger): a twelfth object directory, its source an
# entry of SOURCES in the same way.  Only the two 1x1 blocks and the audio window's transpose run on launchers of lib/obj/ (no new instance there).
OBJ_DIR_SYNC = os.path.join(LIB_DIR, "obj_sync")
SOURCES_SYNC = ["syncnet.hip"]
# The kernels of the bf16 precision of the SyncNet_color handle (tests/kernel_ledger_sync16.py is their ledger): a thirteenth object
# directory, its source an entry of SOURCES in the same way.  What the two precisions share is csrc/syncnet_common.h (an entry of HEADERS).
OBJ_DIR_SYNC16 = os.path.join(LIB_DIR, "obj_sync16")
SOURCES_SYNC16 = ["syncnet_bf16.hip"]
# The kernels of the audio front end, WAV bytes -> the normalised 16 kHz waveform (tests/kernel_ledger_audio.py is their ledger): a
# fourteenth object directory, its source an entry of SOURCES in the same way.
OBJ_DIR_AUDIO = os.path.join(LIB_DIR, "obj_audio")
SOURCES_AUDIO = ["audio.hip"]
# The Motion-JPEG decoder, the baseline decoder's wider sibling: 4:2:2 and grayscale beside 4:4:4 and 4:2:0
# (tests/kernel_ledger_mjpegdec.py is its ledger): a fifteenth object directory, its source an entry of SOURCES in the same way.  What
# the two decoders share is csrc/jpeg_dec_common.h (an entry of HEADERS), in each object's own anonymous namespace.
OBJ_DIR_MJPEGDEC = os.path.join(LIB_DIR, "obj_mjpegdec")
SOURCES_MJPEGDEC = ["jpeg_dec_mjpeg.hip"]
# The kernel that builds the trainer's batches from a resident clip (tests/kernel_ledger_train.py is its ledger): a sixteenth object
# directory, its source an entry of SOURCES in the same way.  Its entry is declared in include/casync_train.h; the 8-bit resize it
# shares with frame_ops.hip is csrc/resize_u8.h (both entries of HEADERS).
OBJ_DIR_TRAIN = os.path.join(LIB_DIR, "obj_train")
SOURCES_TRAIN = ["train_ops.hip"]
# The kernels of the trainer's loss, L1 + VGG19 perceptual with its gradient (tests/kernel_ledger_ploss.py is their ledger): a
# seventeenth object directory, its source an entry of SOURCES in the same way.  Its entries are declared in
# include/casync_ploss.h (an entry of HEADERS); its twelve convs run on launchers of lib/obj/ (no new instance there).
OBJ_DIR_PLOSS = os.path.join(LIB_DIR, "obj_ploss")
SOURCES_PLOSS = ["ploss.hip"]
SOURCES = ["runtime.hip", "gemm.hip", "ops.hip", "ir_fused.hip", "pw_dw.hip", "pw_dw_bf16.hip", "attention.hip", "attention_bf16.hip", "frame_ops.hip", "hubert.hip", "engine.hip"] + SOURCES_DET + SOURCES_DET16 + SOURCES_FACE + SOURCES_NMS + SOURCES_CLIP + SOURCES_JPEG + SOURCES_JPEG420 + SOURCES_JPEGDEC + SOURCES_SYNC + SOURCES_SYNC16 + SOURCES_AUDIO + SOURCES_MJPEGDEC + SOURCES_TRAIN + SOURCES_PLOSS
HEADERS = ["common.h", "handle.h", "ir_common.h", "pw_dw_common.h", "jpeg_enc_common.h", "syncnet_common.h", "jpeg_dec_common.h", "resize_u8.h", os.path.join("..", "..", "include", "casync_hip.h"),
           os.path.join("..", "..", "include", "casync_train.h"), os.path.join("..", "..", "include", "casync_ploss.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the casync HIP engine cannot be built")
    return exe


def _newer(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _header_paths():
    return [os.path.join(CSRC, h) for h in HEADERS]


def is_stale() -> bool:
    """True when the library is missing or older than any of its sources / headers.  A deployment that ships the
    library without csrc/ has nothing to be stale against: missing sources count as "not newer"."""
    return _newer(LIB_PATH, [os.path.join(CSRC, s) for s in SOURCES + SOURCES_HB16 + SOURCES_LMK] + _header_paths())


def source_hash() -> str:
    """sha256 over the HIP sources and headers the library is built from (names + contents, fixed order): written
    into every profiles/*.json by the collection tools and compared by bench.py, so counters collected from one
    version of the kernels are never quoted for another."""
    import hashlib
    h = hashlib.sha256()
    for path in [os.path.join(CSRC, s) for s in SOURCES + SOURCES_HB16 + SOURCES_LMK] + _header_paths():
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


_LLVM_BIN = "/opt/rocm/lib/llvm/bin"
_ERRATUM = None   # compiled lazily: a packed fp32 instruction whose LOW result takes the HIGH half of its SECOND source


def erratum_instructions(obj: str):
    """The gfx950 erratum of round 6 (profiles/r6_two_models.txt section 9; tools/isa_pk_opsel.py is the same check as a tool): such an
    instruction reads that half as zero on lanes 48..63 beside another wave's v_mfma_f32_16x16x32_bf16.  -> [(kernel, instruction)] of one
    object's gfx950 code; [] when the object has no device code or the LLVM binutils are not there."""
    import re
    import tempfile
    global _ERRATUM
    if _ERRATUM is None:
        _ERRATUM = re.compile(r"\b(v_pk_(?:fma|mul|add)_f32)\b([^/]*?op_sel:\[[01],1[^/]*)")
    tools = [os.path.join(_LLVM_BIN, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not all(os.path.exists(t) for t in tools):
        return []
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        if subprocess.run([tools[0], f"--dump-section=.hip_fatbin={fat}", obj], capture_output=True).returncode:
            return []
        if subprocess.run([tools[1], "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"],
                          capture_output=True).returncode:
            return []
        asm = subprocess.run([tools[2], "-d", "--no-show-raw-insn", "-C", co], capture_output=True, text=True).stdout
    hits, cur = [], "?"
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = m.group(1)
            continue
        mm = _ERRATUM.search(line)
        if mm:
            name = cur.replace("(anonymous namespace)::", "").replace("void ", "")
            hits.append((name.split("(")[0], (mm.group(1) + mm.group(2)).strip()))
    return hits


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 (one object per source, in parallel) and link
    calipsync_amd/lib/libcasync_hip.so."""
    if not force and not is_stale():
        return LIB_PATH
    os.makedirs(OBJ_DIR, exist_ok=True)
    os.makedirs(OBJ_DIR_HB16, exist_ok=True)
    os.makedirs(OBJ_DIR_LMK, exist_ok=True)
    os.makedirs(OBJ_DIR_DET, exist_ok=True)
    os.makedirs(OBJ_DIR_DET16, exist_ok=True)
    os.makedirs(OBJ_DIR_FACE, exist_ok=True)
    os.makedirs(OBJ_DIR_NMS, exist_ok=True)
    os.makedirs(OBJ_DIR_CLIP, exist_ok=True)
    os.makedirs(OBJ_DIR_JPEG, exist_ok=True)
    os.makedirs(OBJ_DIR_JPEG420, exist_ok=True)
    os.makedirs(OBJ_DIR_JPEGDEC, exist_ok=True)
    os.makedirs(OBJ_DIR_SYNC, exist_ok=True)
    os.makedirs(OBJ_DIR_SYNC16, exist_ok=True)
    os.makedirs(OBJ_DIR_AUDIO, exist_ok=True)
    os.makedirs(OBJ_DIR_MJPEGDEC, exist_ok=True)
    os.makedirs(OBJ_DIR_TRAIN, exist_ok=True)
    os.makedirs(OBJ_DIR_PLOSS, exist_ok=True)
    # One builder at a time: bench.py --gpus N, torchrun ranks and pytest workers can all reach load() -> build() at
    # once after a checkout; without the lock they compile into the same obj/*.o and link over a library another rank
    # is dlopen-ing.  The link goes to a temporary name and is renamed into place (atomic on one filesystem).
    import fcntl
    with open(os.path.join(LIB_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not is_stale():   # somebody else built it while this process waited
                return LIB_PATH
            return _build_locked(force, verbose)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _build_locked(force: bool, verbose: bool) -> str:
    hipcc = _hipcc()

    def compile_one(src: str):
        obj_dir = OBJ_DIR_HB16 if src in SOURCES_HB16 else OBJ_DIR_LMK if src in SOURCES_LMK else OBJ_DIR_DET if src in SOURCES_DET else \
            OBJ_DIR_DET16 if src in SOURCES_DET16 else OBJ_DIR_FACE if src in SOURCES_FACE else OBJ_DIR_NMS if src in SOURCES_NMS else \
            OBJ_DIR_CLIP if src in SOURCES_CLIP else OBJ_DIR_JPEG if src in SOURCES_JPEG else OBJ_DIR_JPEG420 if src in SOURCES_JPEG420 else \
            OBJ_DIR_JPEGDEC if src in SOURCES_JPEGDEC else OBJ_DIR_SYNC if src in SOURCES_SYNC else OBJ_DIR_SYNC16 if src in SOURCES_SYNC16 else \
            OBJ_DIR_AUDIO if src in SOURCES_AUDIO else OBJ_DIR_MJPEGDEC if src in SOURCES_MJPEGDEC else OBJ_DIR_TRAIN if src in SOURCES_TRAIN else \
            OBJ_DIR_PLOSS if src in SOURCES_PLOSS else OBJ_DIR
        obj = os.path.join(obj_dir, src.replace(".hip", ".o"))
        path = os.path.join(CSRC, src)
        if not force and not _newer(obj, [path] + _header_paths()):
            return obj, None
        cmd = [hipcc] + FLAGS + ["-c", path, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        res = subprocess.run(cmd, capture_output=True, text=True)
        return obj, (res.stdout + res.stderr if res.returncode else None)

    sources = SOURCES + SOURCES_HB16 + SOURCES_LMK
    with ThreadPoolExecutor(max_workers=min(len(sources), os.cpu_count() or 4)) as pool:
        results = list(pool.map(compile_one, sources))
    errors = [err for _, err in results if err]
    if errors:
        raise RuntimeError("hipcc failed:\n" + "\n".join(errors))
    if not os.environ.get("CASYNC_SKIP_ISA_CHECK"):
        # refuse to link a library with the instruction form gfx950 gets wrong beside bf16 matrix instructions (the compiler emits it on
        # its own when a scalar factor lives in the high half of a register pair: pin that scalar in the source, see ir_common.h fma4_scalar)
        bad = [(os.path.basename(obj), k, ins) for obj, _ in results for k, ins in erratum_instructions(obj)]
        if bad:
            raise RuntimeError("gfx950 packed-fp32 op_sel erratum (calipsync_amd/build.py erratum_instructions): the compiler emitted\n" +
                               "\n".join(f"  {o}  {k}:  {ins}" for o, k, ins in bad[:20]))
    tmp = f"{LIB_PATH}.{os.getpid()}.tmp"
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + [obj for obj, _ in results]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise RuntimeError("hipcc link failed:\n" + res.stdout + res.stderr)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force=True, verbose=True))
