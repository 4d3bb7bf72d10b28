/*
 * rsx.h -- C-ABI of the MI355X-native RAW decompression core ("rsx").
 *
 * This is the drop-in boundary behind rawspeed's decompressor classes.  The
 * reference (darktable-org/rawspeed, paths relative to src/librawspeed/)
 * exposes no plugin/FFI interface for decompressors; the seam is created by
 * forwarding from three concrete C++ methods (plus the DNG tile fan-out) into
 * the entry points below.  Every entry point cites the reference interface it
 * replaces.  Plain C types only: no C++ objects, no torch types, no
 * exceptions cross this boundary.  All pointers are borrowed for the duration
 * of the call.  Entry points are re-entrant per context; one context may be
 * shared by several host threads (calls are serialised on the context).
 *
 * Two families of entry points:
 *   - host-pointer calls (rsx_unpack_u16, rsx_ljpeg_decode, rsx_cr2_decode,
 *     rsx_dng_decompress): exactly what the patched reference methods call;
 *     input is pageable host memory, output is the RawImage's host buffer.
 *     They stage H2D / D2H internally.
 *   - device-resident plans (rsx_*_plan_*): inputs and outputs already live in
 *     HBM, launches go to a caller-supplied hipStream_t.  These are what the
 *     roofline measurement and the batched multi-GPU path use.
 */
#ifndef RSX_H
#define RSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSX_ABI_VERSION 4

/* ------------------------------------------------------------------------ */
/* Status codes.  Kernels cannot throw; the C++ forwarding shim converts a   */
/* non-OK status into ThrowRDE / ThrowIOE.                  */
/* ------------------------------------------------------------------------ */
typedef enum rsx_status {
  RSX_OK = 0,
  /* descriptor rejected by the same checks the reference constructor makes
   * (ThrowRDE in UncompressedDecompressor.cpp:106-169,
   * LJpegDecompressor.cpp:52-152, Cr2DecompressorImpl.h:279-363) */
  RSX_ERR_INVALID_ARG = 1,
  /* not enough input (ThrowIOE: UncompressedDecompressor.cpp:52-74,
   * BitStreamer.h:58-59 "Bit stream size is smaller than MaxProcessBytes") */
  RSX_ERR_IO = 2,
  /* "bad Huffman code" (codes/PrefixCodeLookupDecoder.h:152-155) */
  RSX_ERR_BAD_HUFFMAN_CODE = 3,
  /* restart marker missing / wrong (LJpegDecompressor.cpp:288-297) */
  RSX_ERR_RESTART_MARKER = 4,
  /* "Buffer overflow read in BitStreamer" (bitstreams/BitStreamer.h:125-127) */
  RSX_ERR_INPUT_OVERFLOW = 5,
  /* HIP runtime failure (no reference equivalent) */
  RSX_ERR_DEVICE = 6,
  /* valid for the reference but not implemented by this core yet */
  RSX_ERR_UNSUPPORTED = 7,
  RSX_ERR_NOMEM = 8,
  /* AbstractDngDecompressor: at least one tile failed
   * (AbstractDngDecompressor.cpp:247-251 "Too many errors") */
  RSX_ERR_TILE_ERRORS = 9,
  /* "decoded value out of bounds" (PentaxDecompressor.cpp:170-171) */
  RSX_ERR_VALUE_RANGE = 10
} rsx_status;

/* Bit orders; numeric values equal rawspeed::BitOrder
 * (bitstreams/BitStreams.h:27-35). */
typedef enum rsx_bit_order {
  RSX_ORDER_LSB = 0,
  RSX_ORDER_MSB = 1,
  RSX_ORDER_MSB16 = 2,
  RSX_ORDER_MSB32 = 3,
  RSX_ORDER_JPEG = 4
} rsx_bit_order;

/* ------------------------------------------------------------------------ */
/* The RawImage view (common/RawImage.h:289-296): uint16 samples,            */
/* `pitch_bytes` between rows (never assume roundUp(w*bpp,16):               */
/* RawImage.cpp:85-90), `dim_x` x `dim_y` pixels of `cpp` samples each.      */
/* `data` is a host pointer for the host-pointer calls and a device pointer  */
/* for the plan calls.                                                       */
/* ------------------------------------------------------------------------ */
typedef struct rsx_image {
  void* data;
  uint32_t pitch_bytes;
  int32_t dim_x;
  int32_t dim_y;
  int32_t cpp;
  int32_t is_cfa; /* RawImageData::isCFA; only Cr2 sRaw validation reads it */
} rsx_image;

/* ------------------------------------------------------------------------ */
/* Context: one per (host thread group, device).  Owns a HIP stream, staging */
/* buffers and scratch.                                                      */
/* ------------------------------------------------------------------------ */
typedef struct rsx_ctx rsx_ctx;

int rsx_abi_version(void);
const char* rsx_status_string(int status);
/* Number of visible HIP devices (0 when no GPU / no driver). */
int rsx_device_count(void);
/* Creates a context on HIP device `device`.  Fails with RSX_ERR_DEVICE when
 * there is no usable GPU: there is NO CPU fallback in this library. */
int rsx_ctx_create(int device, rsx_ctx** out_ctx);
void rsx_ctx_destroy(rsx_ctx* ctx);
/* Last error text of this context (never NULL). */
const char* rsx_ctx_last_error(const rsx_ctx* ctx);
/* Number of host-pointer calls (rsx_*_decode / rsx_unpack_* / rsx_dng_decompress_* ...)
 * this context has served: lets an integration check that the batched DNG hunk
 *  really makes one call per image. */
uint64_t rsx_ctx_host_calls(const rsx_ctx* ctx);
/* ... and how many of them ran their one large stream in chunks, the upload and the download
 * under the decode (round 6; LJpegDecoder::decode / Cr2LJpegDecoder::decode of a frame whose plan
 * the calling thread's lane holds from the frame before: LJpegDecoder.cpp:161-164,
 * Cr2LJpegDecoder.cpp:150-153 are the callers): a diagnostic, like the count above. */
uint64_t rsx_ctx_chunked_calls(const rsx_ctx* ctx);

/* Optional: page-locked host memory for the host-pointer calls (ABI 4).
 * Those calls take whatever the caller has -- rawspeed's file `Buffer` and the pixel store
 * of RawImageData::createData() (RawImage.cpp:68-100: `data.resize(pitch * dim.y)` over an
 * aligned allocator) are pageable, and a copy from / to pageable memory goes through the
 * driver's staging at a fraction of the link's rate and keeps its calling thread.  An
 * integration that allocates these two buffers here (or registers them after the fact)
 * gets direct DMA and copies that overlap the kernels; nothing else changes, and memory
 * that was not registered keeps working as before.  INTEGRATION.md 6 shows the hunks.
 *   rsx_host_alloc / rsx_host_free          hipHostMalloc'ed block (64-byte aligned and more)
 *   rsx_host_register / rsx_host_unregister  page-lock an existing allocation in place
 * RSX_ERR_NOMEM when the pages cannot be locked (RLIMIT_MEMLOCK, fragmentation): the
 * caller carries on with pageable memory. */
int rsx_host_alloc(rsx_ctx* ctx, size_t bytes, void** out);
int rsx_host_free(rsx_ctx* ctx, void* p);
int rsx_host_register(rsx_ctx* ctx, void* p, size_t bytes);
int rsx_host_unregister(rsx_ctx* ctx, void* p);

/* ------------------------------------------------------------------------ */
/* 1. UncompressedDecompressor                                               */
/*    replaces UncompressedDecompressor::readUncompressedRaw()               */
/*    (decompressors/UncompressedDecompressor.h:75, .cpp:202-268) for the    */
/*    UINT16 packed-integer paths, i.e. decodePackedInt<BitStreamerXXX>      */
/*    (.cpp:188-200) and the 16-bit-LSB copyPixels fast path (.cpp:255-265). */
/*    Fields mirror the constructor (.h:64-66, .cpp:106-169).                */
/* ------------------------------------------------------------------------ */
typedef struct rsx_unpack_desc {
  int32_t crop_x, crop_y; /* iRectangle2D crop.pos (pixels) */
  int32_t crop_w, crop_h; /* iRectangle2D crop.dim (pixels) */
  int32_t input_pitch_bytes;
  int32_t bits_per_pixel; /* 1..16 for UINT16 images */
  int32_t bit_order;      /* rsx_bit_order, JPEG rejected */
} rsx_unpack_desc;

/* Validation only (the reference constructor): RSX_OK or the error the
 * reference would throw.  Needs no GPU. */
int rsx_unpack_validate(const rsx_unpack_desc* d, const rsx_image* img,
                        size_t in_bytes);

int rsx_unpack_u16(rsx_ctx* ctx, const rsx_unpack_desc* d, const uint8_t* in,
                   size_t in_bytes, const rsx_image* img);

/* 1a. The same method on RawImageType::F32 images (.cpp:212-245):            */
/*    bits_per_pixel 32 -> copyPixels (.cpp:213-222), 16 / 24 with MSB or LSB*/
/*    order -> decodePackedFP<Pump, Binary16 | Binary24> (.cpp:171-186,      */
/*    common/FloatingPoint.h:109-145: exact widening to binary32, subnormals */
/*    renormalised, NaN payloads kept).  Anything else is the reference's    */
/*    "Unsupported floating-point input bitwidth/bit packing".  `img->data`  */
/*    holds 4-byte samples; unlike the integer path, decodePackedFP honours  */
/*    crop_x (as a SAMPLE offset, .cpp:181) -- replicated.                   */
int rsx_unpack_f32_validate(const rsx_unpack_desc* d, const rsx_image* img,
                            size_t in_bytes);
int rsx_unpack_f32(rsx_ctx* ctx, const rsx_unpack_desc* d, const uint8_t* in,
                   size_t in_bytes, const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 1b. The fixed-layout entry points of the same class                       */
/*    UncompressedDecompressor::decode8BitRaw<true>()        (.cpp:270-291)  */
/*    UncompressedDecompressor::decode12BitRawWithControl<e>() (.cpp:296-349)*/
/*    UncompressedDecompressor::decode12BitRawUnpackedLeftAligned<e>()       */
/*                                                           (.cpp:356-378)  */
/*    They use only size = crop.dim of the constructor and write from pixel  */
/*    (0,0) of the image, ignoring crop.pos -- replicated.                   */
/*    decode8BitRaw<false>() stores setWithLookUp(byte) instead              */
/*    (common/RawImage.h:335-353) with a random state that starts at 0 and   */
/*    therefore stays 0: the result is a pure function of the byte, passed   */
/*    as `lut` (for a dithering table: tables[2 * v], else tables[v]).       */
/* ------------------------------------------------------------------------ */
typedef enum rsx_unpack_variant {
  RSX_UNPACK_8BIT_RAW = 0,
  RSX_UNPACK_12BIT_WITH_CONTROL = 1,
  RSX_UNPACK_12BIT_UNPACKED_LEFT_ALIGNED = 2,
  RSX_UNPACK_8BIT_LOOKUP = 3 /* decode8BitRaw<false> */
} rsx_unpack_variant;

typedef struct rsx_unpack_variant_desc {
  int32_t variant;    /* rsx_unpack_variant */
  int32_t big_endian; /* template parameter Endianness e (ignored for 8-bit) */
  int32_t w, h;       /* size.x, size.y */
  uint16_t lut[256];  /* RSX_UNPACK_8BIT_LOOKUP only */
} rsx_unpack_variant_desc;

int rsx_unpack_variant_validate(const rsx_unpack_variant_desc* d,
                                const rsx_image* img, size_t in_bytes);
int rsx_unpack_variant_u16(rsx_ctx* ctx, const rsx_unpack_variant_desc* d,
                           const uint8_t* in, size_t in_bytes,
                           const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* Huffman table exactly as the DHT payload the host already parsed          */
/* (codes/HuffmanCode.h:99-166): 16 counts + the code values (= SSSS         */
/* difference categories, each <= 16 in full-decode mode,                    */
/* codes/AbstractPrefixCodeTranscoder.h:71-84).  The canonical code is       */
/* re-derived on our side; the reference's LUT memory is never read.         */
/* ------------------------------------------------------------------------ */
#define RSX_MAX_CODE_VALUES 162 /* codes/AbstractPrefixCode.h BaselineCodeTag */
typedef struct rsx_huff_table {
  uint8_t n_codes_per_length[16]; /* index 0 = code length 1 */
  uint8_t code_values[RSX_MAX_CODE_VALUES];
  uint8_t n_code_values;
  uint8_t fix_dng_bug16; /* AbstractPrefixCodeDecoder.h:58-62 */
} rsx_huff_table;

#define RSX_MAX_COMPONENTS 4

/* ------------------------------------------------------------------------ */
/* 2. LJpegDecompressor                                                      */
/*    replaces LJpegDecompressor::decode() (LJpegDecompressor.h:94,          */
/*    .cpp:341-370 -> decodeN .cpp:254-339 -> decodeRowN .cpp:184-251).      */
/*    Fields mirror the constructor (.h:89-93, .cpp:52-152).                 */
/* ------------------------------------------------------------------------ */
typedef struct rsx_ljpeg_desc {
  int32_t tile_x, tile_y, tile_w, tile_h; /* imgFrame, pixels */
  int32_t mcu_w, mcu_h;                   /* Frame::mcu */
  int32_t frame_w, frame_h;               /* Frame::dim, in MCUs */
  int32_t n_comp;                         /* rec.size() == mcu_w*mcu_h */
  int32_t rows_per_restart_interval;      /* numLJpegRowsPerRestartInterval */
  uint16_t init_pred[RSX_MAX_COMPONENTS]; /* PerComponentRecipe::initPred */
  uint8_t table_index[RSX_MAX_COMPONENTS]; /* PerComponentRecipe::ht -> tables[] */
  int32_t n_tables;
  rsx_huff_table tables[RSX_MAX_COMPONENTS];
} rsx_ljpeg_desc;

int rsx_ljpeg_validate(const rsx_ljpeg_desc* d, const rsx_image* img,
                       size_t in_bytes);

/* `in` = entropy-coded data from just after the SOS header to the end of the
 * tile buffer (what LJpegDecoder::decodeScan passes, LJpegDecoder.cpp:161-164).
 * `consumed` = ByteStream::size_type return value of decode() (closed form:
 * SURVEY.md A.6). */
int rsx_ljpeg_decode(rsx_ctx* ctx, const rsx_ljpeg_desc* d, const uint8_t* in,
                     size_t in_bytes, const rsx_image* img,
                     uint32_t* consumed);

/* ------------------------------------------------------------------------ */
/* 3. Cr2Decompressor<PrefixCodeDecoder<>>                                   */
/*    replaces Cr2Decompressor::decompress() (Cr2Decompressor.h:174,         */
/*    Cr2DecompressorImpl.h:471-485 -> decompressN_X_Y :396-468).            */
/*    Fields mirror the constructor (Cr2Decompressor.h:168-172,              */
/*    Cr2DecompressorImpl.h:279-363).                                        */
/* ------------------------------------------------------------------------ */
typedef struct rsx_cr2_desc {
  int32_t n_comp, x_s_f, y_s_f; /* format tuple */
  int32_t frame_w, frame_h;     /* iPoint2D frame (as passed, before /X_S_F) */
  int32_t num_slices, slice_width, last_slice_width; /* Cr2SliceWidths */
  uint16_t init_pred[RSX_MAX_COMPONENTS];
  uint8_t table_index[RSX_MAX_COMPONENTS];
  int32_t n_tables;
  rsx_huff_table tables[RSX_MAX_COMPONENTS];
} rsx_cr2_desc;

int rsx_cr2_validate(const rsx_cr2_desc* d, const rsx_image* img,
                     size_t in_bytes);

int rsx_cr2_decode(rsx_ctx* ctx, const rsx_cr2_desc* d, const uint8_t* in,
                   size_t in_bytes, const rsx_image* img, uint32_t* consumed);

/* ------------------------------------------------------------------------ */
/* 3a. Cr2sRawInterpolator                                                   */
/*    replaces Cr2sRawInterpolator::interpolate(version)                     */
/*    (interpolators/Cr2sRawInterpolator.h:49, .cpp:510-542 ->               */
/*    interpolate_422<v> :95-186 / interpolate_420<v> :188-460,              */
/*    YUV_TO_RGB<v> :470-506): the step Cr2Decoder runs right after the sRaw */
/*    decompress (Cr2Decoder.cpp:585-625).  `in` is the decoded subsampled   */
/*    image (cpp 1: groups of Y Y Cb Cr or Y Y Y Y Cb Cr), `out` the         */
/*    interpolated one (cpp 3, 2 * groups pixels wide, subsampling_y * rows  */
/*    high).  All arithmetic is the reference's int arithmetic.              */
/* ------------------------------------------------------------------------ */
typedef struct rsx_sraw_desc {
  int32_t version;        /* 0, 1, 2 (0 only with subsampling_y == 1) */
  int32_t subsampling_y;  /* 1: 4:2:2 (groups of 4), 2: 4:2:0 (groups of 6); x is always 2 */
  int32_t sraw_coeffs[3];
  int32_t hue;
} rsx_sraw_desc;

int rsx_sraw_validate(const rsx_sraw_desc* d, const rsx_image* in, const rsx_image* out);
int rsx_sraw_interpolate(rsx_ctx* ctx, const rsx_sraw_desc* d, const rsx_image* in,
                         const rsx_image* out);

/* ------------------------------------------------------------------------ */
/* 3b. NikonDecompressor                                                     */
/*    replaces NikonDecompressor::decompress(input, uncorrectedRawValues)    */
/*    (decompressors/NikonDecompressor.h:57, .cpp:541-560 ->                 */
/*    decompress<Huffman>(bits, start_y, end_y) :515-539).  The constructor  */
/*    (.cpp:473-513: metadata parsing, createCurve :381-445) stays on the    */
/*    host; its results are the fields below.                                */
/*      - bit stream: BitStreamerMSB over `in` (no byte stuffing, no markers)*/
/*      - tables[0] = nikon_tree[huffSelect] decoded by PrefixCodeDecoder<>  */
/*        (full decode, no DNG bug); rows >= split (if split != 0) use       */
/*        tables[1] = nikon_tree[huffSelect + 1] with the "lossy after       */
/*        split" semantics of NikonLASDecompressor::decodeDifference         */
/*        (.cpp:331-376): code value v -> len = v & 15, shl = v >> 4,        */
/*        len - shl raw bits, diff = ((bits << 1) + 1) << shl >> 1, sign     */
/*        extension on bit len-1; v == 16 -> -32768                          */
/*      - predictor: int accumulators pred[col & 1] seeded from              */
/*        pUp[row & 1][col & 1], which the first two columns update          */
/*      - output: clampBits(pred, 15), then RawImageData::setWithLookUp      */
/*        (common/RawImage.h:335-353): as is when uncorrected_raw_values,    */
/*        else through the dithering TableLookUp built from `curve`          */
/*        (common/TableLookUp.cpp:50-84) with the serial random state seeded */
/*        from bits.peekBits(24) (.cpp:549)                                  */
/* ------------------------------------------------------------------------ */
typedef struct rsx_nikon_desc {
  int32_t bits_ps; /* 12 or 14 (.cpp:485-491) */
  int32_t split;   /* 0 = no split (already clamped against dim.y, .cpp:511-512) */
  int32_t p_up[2][2]; /* pUp[row & 1][col & 1] (.cpp:506-509) */
  int32_t uncorrected_raw_values;
  int32_t curve_size;    /* entries of `curve` (1 .. 65536) */
  const uint16_t* curve; /* host pointer; copied during the call */
  rsx_huff_table tables[2];
} rsx_nikon_desc;

int rsx_nikon_validate(const rsx_nikon_desc* d, const rsx_image* img);

int rsx_nikon_decompress(rsx_ctx* ctx, const rsx_nikon_desc* d, const uint8_t* in,
                         size_t in_bytes, const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 3c. PentaxDecompressor                                                    */
/*    replaces PentaxDecompressor::decompress(ByteStream data)               */
/*    (decompressors/PentaxDecompressor.h, .cpp:152-176): BitStreamerMSB,    */
/*    one PrefixCodeDecoder<> (the legacy tree or the one the constructor    */
/*    derives from the makernote, .cpp:69-150 -- stays on the host),         */
/*    pred[col & 1] += diff with both predictors starting from the pixels    */
/*    two rows up (0 for the first two rows); a value outside [0, 65535]     */
/*    is RSX_ERR_VALUE_RANGE.                                                */
/* ------------------------------------------------------------------------ */
typedef struct rsx_pentax_desc {
  rsx_huff_table table;
} rsx_pentax_desc;

int rsx_pentax_validate(const rsx_pentax_desc* d, const rsx_image* img);
int rsx_pentax_decompress(rsx_ctx* ctx, const rsx_pentax_desc* d, const uint8_t* in,
                          size_t in_bytes, const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 3d. SamsungV1Decompressor                                                 */
/*    replaces SamsungV1Decompressor::decompress()                           */
/*    (decompressors/SamsungV1Decompressor.cpp:81-140): BitStreamerMSB, a    */
/*    fixed prefix code given as (encLen, diffLen) pairs that fill a 10-bit  */
/*    table in order (.cpp:88-117) -- NOT a canonical JPEG code, so it is    */
/*    handed over in that form --, samsungDiff (.cpp:63-79: fill(23),        */
/*    diffLen raw bits, sign extension), and the two-rows-up predictor of    */
/*    PentaxDecompressor with values limited to `bits` bits (.cpp:129-136).  */
/* ------------------------------------------------------------------------ */
#define RSX_SAMSUNG_V1_MAX_ENTRIES 32
typedef struct rsx_samsung_v1_desc {
  int32_t bits;      /* the constructor accepts only 12 (.cpp:53-54) */
  int32_t n_entries; /* 14 in the reference */
  uint8_t enc_len[RSX_SAMSUNG_V1_MAX_ENTRIES];  /* tab[i][0], 1..10 */
  uint8_t diff_len[RSX_SAMSUNG_V1_MAX_ENTRIES]; /* tab[i][1], 0..13 */
} rsx_samsung_v1_desc;

int rsx_samsung_v1_validate(const rsx_samsung_v1_desc* d, const rsx_image* img);
int rsx_samsung_v1_decompress(rsx_ctx* ctx, const rsx_samsung_v1_desc* d,
                              const uint8_t* in, size_t in_bytes, const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 3g. SamsungV2Decompressor                                                 */
/*    replaces SamsungV2Decompressor::decompress()                           */
/*    (decompressors/SamsungV2Decompressor.h:74, .cpp:340-343: decompressRow */
/*    for every row, .cpp:312-338).  The descriptor is what the constructor  */
/*    (.cpp:85-141) reads from the 16-byte header -- bitDepth, width,        */
/*    height, optflags, initVal -- and `in` is its member `data`: the bytes   */
/*    behind that header.  Every row is a BitStreamerMSB32 of its own that   */
/*    starts at the next 16-byte boundary of `data` (.cpp:314-318); a row is */
/*    width / 16 blocks (processBlock .cpp:312-327: prepareBaselineValues    */
/*    .cpp:152-230, decodeDiffLengths .cpp:232-277, decodeDifferences        */
/*    .cpp:279-311), pixels are clampBits(baseline + difference, bitDepth).  */
/*    rsx_samsung_v2_validate = the constructor's checks (.cpp:88-100,       */
/*    :123-125, :134-139).  Statuses: what the reference throws, in its      */
/*    order -- RSX_ERR_INVALID_ARG for its ThrowRDEs (.cpp:172-173, :191-    */
/*    192, :212-219, :258-259, :271-272), RSX_ERR_IO / RSX_ERR_INPUT_        */
/*    OVERFLOW for the stream running out; the image is unspecified then.    */
/* ------------------------------------------------------------------------ */
typedef struct rsx_samsung_v2_desc {
  int32_t bit_depth;  /* bitDepth: 12 or 14 */
  int32_t width;      /* multiple of 16, <= 6496 */
  int32_t height;     /* <= 4336 */
  uint32_t optflags;  /* OptFlags (.cpp:46-54): 1 SKIP, 2 MV, 4 QP */
  uint32_t init_val;  /* initVal (14 bits) */
} rsx_samsung_v2_desc;

int rsx_samsung_v2_validate(const rsx_samsung_v2_desc* d, const rsx_image* img);
int rsx_samsung_v2_decompress(rsx_ctx* ctx, const rsx_samsung_v2_desc* d, const uint8_t* in,
                              size_t in_bytes, const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 3e. HasselbladDecompressor                                                */
/*    replaces HasselbladDecompressor::decompress()                          */
/*    (decompressors/HasselbladDecompressor.h:53, .cpp:71-100): BitStreamer- */
/*    MSB32 (little-endian 32-bit words, MSB first, no stuffing), pixels     */
/*    coded two at a time as [len1 code][len2 code][len1 bits][len2 bits]    */
/*    with one PrefixCodeDecoder<> used for its code VALUES only             */
/*    (decodeCodeValue), getBits (.cpp:60-69: JPEG sign extension, all-ones  */
/*    16-bit field = -32768), both predictors restart from initPred on every */
/*    row, results stored mod 2^16.  Returns getStreamPosition().            */
/* ------------------------------------------------------------------------ */
typedef struct rsx_hasselblad_desc {
  rsx_huff_table table; /* rec.ht (values = difference lengths 0..16) */
  uint16_t init_pred;   /* rec.initPred */
} rsx_hasselblad_desc;

int rsx_hasselblad_validate(const rsx_hasselblad_desc* d, const rsx_image* img);
int rsx_hasselblad_decompress(rsx_ctx* ctx, const rsx_hasselblad_desc* d, const uint8_t* in,
                              size_t in_bytes, const rsx_image* img, uint32_t* consumed);

/* ------------------------------------------------------------------------ */
/* 3f. SonyArw1Decompressor                                                  */
/*    replaces SonyArw1Decompressor::decompress(ByteStream)                  */
/*    (decompressors/SonyArw1Decompressor.h:44, .cpp:59-93): BitStreamerMSB, */
/*    a fixed prefix code for the difference length (2 bits -> 4 - x; "011"  */
/*    = 0; "00" + k zeros + "1" = 4 + k, capped at 17, .cpp:76-83), JPEG     */
/*    sign extension of the difference bits, ONE predictor running through   */
/*    the whole image in decode order: columns right to left, in each column */
/*    the even rows top to bottom and then the odd rows (.cpp:68-74).  A     */
/*    value outside 0..4095 is an error (isIntN(pred, 12), .cpp:88-89).  The */
/*    constructor's checks (cpp 1, U16, w <= 4600, h <= 3072, h even,        */
/*    .cpp:39-51) are rsx_sony_arw1_validate.  No parameters besides the     */
/*    image: the code is fixed.                                              */
/* ------------------------------------------------------------------------ */
int rsx_sony_arw1_validate(const rsx_image* img);
int rsx_sony_arw1_decompress(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes,
                             const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 3h. PhaseOneDecompressor                                                  */
/*    replaces PhaseOneDecompressor::decompress()                            */
/*    (decompressors/PhaseOneDecompressor.cpp:156-170 -> decompressStrip     */
/*    :85-136 for every strip).  IiqDecoder keeps its host work: container   */
/*    parsing, computeSripes (IiqDecoder.cpp:75-118: a strip runs from its   */
/*    offset to the next larger one, the last to the end of raw_data); the   */
/*    pixel passes of CorrectPhaseOneC have a device path of their own       */
/*    (section 3n: rsx_phase_one_decompress_corrected decodes, corrects and  */
/*    downloads once), its parse, the defect list and correctBadColumn stay  */
/*    on the host.  One strip per image row; each is a BitStreamerMSB32      */
/*    over exactly its own bytes (bytes behind the strip read as zero, not   */
/*    as the next row).  Per row: pred[2] = {0, 0}; for col < (w & ~7),      */
/*    col % 8 == 0, a header for len[0] then len[1] (up to five 0-bits up to */
/*    a 1-bit; j zeros > 0: one more bit b, len = {8,7,6,9,11,10,5,12,14,13} */
/*    [2 (j - 1) + b]; j == 0: len kept); the last w % 8 pixels have len 14; */
/*    len 14 = a raw 16-bit value that resets pred[col & 1], else            */
/*    pred += bits(len) + 1 - (1 << (len - 1)); pixel = uint16(pred).        */
/*    rsx_phase_one_validate = the constructor's checks (:43-84: cpp 1,      */
/*    dim > 0, dim_x even, dim_x <= 11976, dim_y <= 8854, exactly one strip  */
/*    per row 0 .. dim_y - 1) plus: every strip lies inside [0, in_bytes)    */
/*    -> RSX_ERR_INVALID_ARG.  Per-row statuses (the first that applies):    */
/*      RSX_ERR_IO               strip shorter than 4 bytes ("Bit stream     */
/*                               size is smaller than MaxProcessBytes",      */
/*                               bitstreams/BitStreamer.h:58-59)             */
/*      RSX_ERR_BAD_HUFFMAN_CODE a 1-bit inside a length prefix at col 0     */
/*                               ("Can not initialize lengths", :107-108)    */
/*      RSX_ERR_INPUT_OVERFLOW   a refill more than 8 bytes past the strip   */
/*                               (BitStreamer.h:124-127): with c the start   */
/*                               bit of pixel w - 1, 4 ceil(c / 32) > size+8 */
/*    Any failing row fails the decode ("Too many errors", :156-170); the    */
/*    call returns the status of the lowest-numbered failing row, and        */
/*    through host pointers leaves the caller's image untouched then.        */
/*    `strip_status` (may be NULL) gets one status per image row.            */
/* ------------------------------------------------------------------------ */
typedef struct rsx_phase_one_strip {
  uint32_t n;        /* image row */
  uint32_t reserved;
  uint64_t offset;   /* byte offset of the strip inside `in` */
  uint64_t bytes;    /* strip size (next larger offset - offset) */
} rsx_phase_one_strip;

int rsx_phase_one_validate(int n_strips, const rsx_phase_one_strip* strips, size_t in_bytes,
                           const rsx_image* img);
int rsx_phase_one_decompress(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes, int n_strips,
                             const rsx_phase_one_strip* strips, const rsx_image* img,
                             int32_t* strip_status);

/* ------------------------------------------------------------------------ */
/* 3i. SonyArw2Decompressor                                                  */
/*    replaces SonyArw2Decompressor::decompress()                            */
/*    (decompressors/SonyArw2Decompressor.cpp:136-148 -> decompressRow       */
/*    :57-120 for every row).  ArwDecoder keeps its host work: the container */
/*    (ArwDecoder.cpp:165-260), decodeCurve (:147-162) and the curve guard   */
/*    (common/RawImage.h:355-383) that installs mRaw->table before the call. */
/*    Row y is exactly the bytes [y w, (y + 1) w) (a BitStreamerLSB); its    */
/*    first 24 bits seed the dither generator.  16-byte blocks of 16 pixels; */
/*    block b holds the columns 32 (b >> 1) + (b & 1) + 2 i, i = 0..15:      */
/*    bits 0-10 max, 11-21 min, 22-25 imax, 26-29 imin, fourteen 7-bit       */
/*    fields from bit 30, taken in order by the pixels i != imax, imin:      */
/*    p = min(0x7ff, (field << sh) + min), sh = the least s in 0..4 with     */
/*    s == 4 or (0x80 << s) > max - min; pixel imax = max, pixel imin = min. */
/*    The value stored is setWithLookUp(p << 1) (RawImage.h:335-353) with    */
/*    the table `desc` describes -- mRaw->table as TableLookUp holds it      */
/*    (common/TableLookUp.cpp), compare decode8BitRaw<false>'s lut in 1b:    */
/*      RSX_ARW2_TABLE_NONE    no table (uncorrectedRawValues): p << 1       */
/*      RSX_ARW2_TABLE_PLAIN   table[p << 1] (4096 entries read)             */
/*      RSX_ARW2_TABLE_DITHER  base = table[2 v], delta = table[2 v + 1],    */
/*                             v = p << 1 (8192 entries read): base + ((delta */
/*                             (r & 2047) + 1024) >> 12), then r = 15700     */
/*                             (r & 65535) + (r >> 16), once a pixel in      */
/*                             decode order (pixel i of block b: step 16 b+i)*/
/*    The table is copied during the call (or at plan creation).             */
/*    rsx_sony_arw2_validate: desc NULL, an unknown table_mode, or a NULL    */
/*    table with a mode other than NONE -> RSX_ERR_INVALID_ARG; then the     */
/*    constructor's checks in its order (:40-54): cpp 1, dim > 0,            */
/*    dim_x % 32 == 0, dim_x <= 9600, dim_y <= 6376 (and pitch_bytes >=      */
/*    2 dim_x) -> RSX_ERR_INVALID_ARG; in_bytes < dim_x dim_y                */
/*    (input.peekStream) -> RSX_ERR_IO.  Bytes behind dim_x dim_y are not    */
/*    read; a job consumes exactly dim_x dim_y bytes.                        */
/*    A block with imax == imin fails its row ("ARW2 invariant failed",      */
/*    :85-86; row status RSX_ERR_INVALID_ARG), and any failing row fails the */
/*    call ("Too many errors", :143-147 -> RSX_ERR_TILE_ERRORS).  Through    */
/*    host pointers the caller's image is then left untouched.               */
/*    `row_status` (may be NULL) gets one status per image row.              */
/* ------------------------------------------------------------------------ */
enum {
  RSX_ARW2_TABLE_NONE = 0,
  RSX_ARW2_TABLE_PLAIN = 1,
  RSX_ARW2_TABLE_DITHER = 2
};

typedef struct rsx_sony_arw2_desc {
  int32_t table_mode;    /* RSX_ARW2_TABLE_* */
  int32_t reserved;
  const uint16_t* table; /* TableLookUp::tables: 4096 (PLAIN) / 8192 (DITHER) entries */
} rsx_sony_arw2_desc;

int rsx_sony_arw2_validate(const rsx_sony_arw2_desc* desc, const rsx_image* img,
                           size_t in_bytes);
int rsx_sony_arw2_decompress(rsx_ctx* ctx, const rsx_sony_arw2_desc* desc, const uint8_t* in,
                             size_t in_bytes, const rsx_image* img, int32_t* row_status);

/* ------------------------------------------------------------------------ */
/* 3j. PanasonicV5Decompressor, PanasonicV6Decompressor,                     */
/*     PanasonicV7Decompressor                                               */
/*    replaces PanasonicV5Decompressor::decompress()                         */
/*    (decompressors/PanasonicV5Decompressor.cpp:253-264 -> processBlock     */
/*    :209-234), PanasonicV6Decompressor::decompress() (PanasonicV6-         */
/*    Decompressor.cpp:250-261 -> decompressBlock :176-220) and              */
/*    PanasonicV7Decompressor::decompress() (PanasonicV7Decompressor.cpp     */
/*    :91-104 -> decompressBlock :67-74).  Rw2Decoder keeps its host work:   */
/*    the container, the version switch (decoders/Rw2Decoder.cpp:138-175)    */
/*    and the metadata.  PanasonicV4Decompressor is NOT covered (it appends  */
/*    to mRaw->mBadPixelPositions, which has no shape here yet).             */
/*    The image is a run of 16-byte packets, each read as one 128-bit        */
/*    little-endian number (bit 0 = the LSB of byte 0).  Packet p holds the  */
/*    pixels [p n, (p + 1) n) in row-major order:                            */
/*      version 7, bps 14, n = 9   pixel i = bits [14 i, 14 i + 14); packet  */
/*                                 p at byte 16 p                            */
/*      version 5, bps 12, n = 10  pixel i = bits [bps i, bps i + bps).  The */
/*      version 5, bps 14, n = 9   input is cut into blocks of 0x4000 bytes  */
/*                                 = 1024 packets; a block's bytes [0x1FF8,  */
/*                                 0x4000) are read first, then [0, 0x1FF8): */
/*                                 packet q of a block starts at its byte    */
/*                                 (16 q + 0x1FF8) mod 0x4000, and packet    */
/*                                 512 wraps around the block's end          */
/*      version 6, bps 14, n = 11  from bit 128 down: two pixels of bps      */
/*      version 6, bps 12, n = 14  bits, then per three pixels a 2-bit scale */
/*                                 b (3 means 4) and three fields of 10 (8)  */
/*                                 bits; packet p at byte 16 p.  Per column  */
/*                                 parity, e = the field while no non-zero   */
/*                                 field was met (a zero field repeats the   */
/*                                 parity's last e), afterwards e = (field   */
/*                                 << b) + max(0, last e - (Z << b)) with    */
/*                                 Z = 0x200 (0x80), the second term only    */
/*                                 for b < 4.  Stored: e - 15, or 0 for      */
/*                                 e < 15; NOT clamped to bps bits.          */
/*    rsx_panasonic_validate: desc NULL or a version other than 5, 6, 7 ->   */
/*    RSX_ERR_INVALID_ARG; Rw2Decoder's own rules (:155-157, :165-167):      */
/*    version 6 takes bps 12 or 14, version 7 bps 14; then the constructors' */
/*    checks in their order (V5 :74-108, V6 :141-169, V7 :44-60): cpp 1,     */
/*    bps 12 or 14, dim > 0 and dim_x % n == 0 (and pitch_bytes >= 2 dim_x), */
/*    then "Insufficient count of input blocks": in_bytes / 16 < packets     */
/*    (V6, V7), in_bytes / 0x4000 < ceil(packets / 1024) (V5).  All of them  */
/*    are ThrowRDE -> RSX_ERR_INVALID_ARG.  A job consumes what peekStream   */
/*    takes, 16 packets resp. 0x4000 ceil(packets / 1024) bytes; a count     */
/*    that does not fit 32 bits -> RSX_ERR_UNSUPPORTED.  Bytes behind the    */
/*    consumed count are not read.  Nothing in the data can fail             */
/*    (decompress() is noexcept), so there is no per-row status.             */
/* ------------------------------------------------------------------------ */
typedef struct rsx_panasonic_desc {
  int32_t version; /* PANASONIC_RAWFORMAT: 5, 6 or 7 */
  int32_t bps;     /* PANASONIC_BITSPERSAMPLE */
} rsx_panasonic_desc;

int rsx_panasonic_validate(const rsx_panasonic_desc* desc, const rsx_image* img,
                           size_t in_bytes);
int rsx_panasonic_decompress(rsx_ctx* ctx, const rsx_panasonic_desc* desc, const uint8_t* in,
                             size_t in_bytes, const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 3k. SamsungV0Decompressor                                                 */
/*    replaces SamsungV0Decompressor::decompress()                           */
/*    (decompressors/SamsungV0Decompressor.cpp:92-102 -> decompressStrip     */
/*    :110-204 for every row, then the swap).  SrwDecoder keeps its host     */
/*    work (decoders/SrwDecoder.cpp:85-106): tag 40976 holds the file offset */
/*    of dim_y little-endian u32 row offsets (`bso`), `in` is the strip      */
/*    (`bsr`).  Row y is the bytes [off[y], off[y + 1]) of `in`, off[dim_y]  */
/*    = in_bytes; each is a BitStreamerMSB32 over exactly its own bytes      */
/*    (bytes behind the row read as zero, not as the next row).  len[0..3]   */
/*    start at 7 for rows 0 and 1, at 4 otherwise.  Per block of 16 columns: */
/*    1 bit dir, four 2-bit ops, then for i = 0..3: op 3 len[i] = 4 bits,    */
/*    op 2 len[i]--, op 1 len[i]++, op 0 keep; the 8 even pixels (len[c>>3]) */
/*    and the 8 odd ones (len[2 | c >> 3]) follow, each signExtend(bits(n),  */
/*    n), 0 for n = 0.  dir 0: pixel = adj + the block's left neighbour of   */
/*    the same parity, out(row, col - 2) resp. out(row, col - 1), 128 at     */
/*    col 0 -- one predictor for all eight; pixels at col + c >= dim_x are   */
/*    read, not written.  dir 1: even pixel = adj + out(row - 1, col + c),   */
/*    odd pixel = adj + out(row - 2, col + c).  All mod 2^16.  At the end    */
/*    out(row, col + 1) <-> out(row + 1, col) for even row < dim_y - 1 and   */
/*    even col < dim_x - 1.                                                  */
/*    rsx_samsung_v0_validate = the constructor's checks, then               */
/*    computeStripes' (:44-90), in their order: cpp 1, 16 <= dim_x <= 5546,  */
/*    1 <= dim_y <= 3714 (and pitch_bytes >= 2 dim_x) -> RSX_ERR_INVALID_ARG;*/
/*    in_bytes >= 4 GiB -> RSX_ERR_UNSUPPORTED (the offsets are 32-bit);     */
/*    n_offsets < dim_y (peekStream) -> RSX_ERR_IO; off[0] > in_bytes        */
/*    (skipBytes) -> RSX_ERR_IO; then pair by pair: off[y] >= off[y + 1]     */
/*    ("Line offsets are out of sequence or slice is empty") ->              */
/*    RSX_ERR_INVALID_ARG, off[y + 1] > in_bytes (getStream) -> RSX_ERR_IO.  */
/*    Offsets behind the first dim_y are not read.                           */
/*    Per-row statuses, the first exception of the row in stream order:      */
/*      RSX_ERR_IO              row shorter than 4 bytes ("Bit stream size   */
/*                              is smaller than MaxProcessBytes")            */
/*      RSX_ERR_INPUT_OVERFLOW  a refill more than 8 bytes past the row      */
/*                              (BitStreamer.h:100-132): a request of n bits */
/*                              after c consumed ones -- 32 at a block's     */
/*                              start, 4 per op 3, len per pixel with        */
/*                              len > 0 -- with 4 (ceil((c + n) / 32) - 1)   */
/*                              > size + 8                                   */
/*      RSX_ERR_VALUE_RANGE     a length below 0 or above 16 (:147-150)      */
/*      RSX_ERR_INVALID_ARG     dir 1 in rows 0, 1 or in the last block of a */
/*                              row (:156-160)                               */
/*    The reference throws at the first failing row; the call returns the    */
/*    status of the lowest-numbered failing row, and through host pointers   */
/*    leaves the caller's image untouched then.                              */
/*    `row_status` (may be NULL) gets one status per image row.              */
/* ------------------------------------------------------------------------ */
int rsx_samsung_v0_validate(const uint32_t* row_offsets, int n_offsets, size_t in_bytes,
                            const rsx_image* img);
int rsx_samsung_v0_decompress(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes,
                              const uint32_t* row_offsets, int n_offsets,
                              const rsx_image* img, int32_t* row_status);

/* ------------------------------------------------------------------------ */
/* 3l. PanasonicV4Decompressor                                               */
/*    replaces PanasonicV4Decompressor::decompress()                         */
/*    (decompressors/PanasonicV4Decompressor.cpp:268-275 -> processBlock     */
/*    :220-241 -> processPixelPacket :173-218).  Rw2Decoder keeps its host   */
/*    work; it builds the decompressor for PANASONIC_RAWFORMAT 4 with        */
/*    section_split_offset 0x1FF8 (decoders/Rw2Decoder.cpp:140-146) and for  */
/*    old-style files without PANASONIC_STRIPOFFSET with 0 (:79-120).        */
/*    The input is cut into blocks of 0x4000 bytes = 1024 packets of 16      */
/*    bytes (split 0: the last block may be partial); a block's bytes        */
/*    [split, 0x4000) are read first, then [0, split): packet q of a block   */
/*    starts at its byte (16 q + split) mod 0x4000, and with 0x1FF8 packet   */
/*    512 wraps around the block's end.  A packet is one 128-bit little-     */
/*    endian number read from bit 128 down and holds 14 pixels of one row    */
/*    (dim_x % 14 == 0).  Per pixel p, column parity c = p & 1: in front of  */
/*    the pixels 2, 5, 8, 11 a 2-bit scale b, sh = 4 >> (3 - b); then 8 bits */
/*    f.  While the parity has met no non-zero f: nonz = f, and for f != 0   */
/*    or p > 11 four more bits g follow, pred = f << 4 | g.  Afterwards, for */
/*    f != 0: pred -= 0x80 << sh; if pred < 0 or sh == 4, pred &= (1 << sh)  */
/*    - 1; pred += f << sh.  The pixel is uint16(pred).  Every parity reads  */
/*    exactly one g, so a packet always takes its 128 bits, and pred stays   */
/*    in 0 .. 16287.  Nothing in the data can fail (decompress() is          */
/*    noexcept), so there is no per-row status.                              */
/*    rsx_panasonic_v4_validate = the constructor's checks (:49-86) in their */
/*    order: desc NULL, cpp != 1, dim <= 0 or dim_x % 14 != 0 (or            */
/*    pitch_bytes < 2 dim_x), section_split_offset > 0x4000, bufSize >       */
/*    UINT32_MAX -> RSX_ERR_INVALID_ARG, where bufSize = 16 dim_x dim_y / 14 */
/*    for split 0 and that rounded up to whole blocks otherwise; in_bytes <  */
/*    bufSize (peekStream) -> RSX_ERR_IO; then a split other than 0 and      */
/*    0x1FF8 -> RSX_ERR_UNSUPPORTED (no caller passes one).  A job consumes  */
/*    bufSize; bytes behind it are not read.                                 */
/*    The bad-pixel list: with zero_is_bad the reference appends row << 16 | */
/*    col of every pixel with pred == 0 -- exactly the zero pixels of the    */
/*    image -- to mRaw->mBadPixelPositions, per thread in completion order.  */
/*    Here the entries come back in ascending order (the reference's order   */
/*    on one thread).  *n_bad (may be NULL) is always the exact count; 0     */
/*    with zero_is_bad == 0, when nothing is collected.  When n_bad exceeds  */
/*    the capacity the image is still complete and correct, the call (the    */
/*    job) reports RSX_ERR_UNSUPPORTED and the list's contents are           */
/*    unspecified.  `bad` NULL with bad_cap 0 is allowed.                    */
/* ------------------------------------------------------------------------ */
typedef struct rsx_panasonic_v4_desc {
  uint32_t section_split_offset; /* 0 (old-style files) or 0x1FF8 (PANASONIC_RAWFORMAT 4) */
  int32_t zero_is_bad;           /* !hints.contains("zero_is_not_bad") */
} rsx_panasonic_v4_desc;

int rsx_panasonic_v4_validate(const rsx_panasonic_v4_desc* desc, const rsx_image* img,
                              size_t in_bytes);
int rsx_panasonic_v4_decompress(rsx_ctx* ctx, const rsx_panasonic_v4_desc* desc, const uint8_t* in,
                                size_t in_bytes, const rsx_image* img, uint32_t* bad,
                                uint32_t bad_cap, uint64_t* n_bad);

/* ------------------------------------------------------------------------ */
/* 3m. NefDecoder::DecodeNikonSNef                                           */
/*    replaces the pixel loop of NefDecoder::DecodeNikonSNef                 */
/*    (decoders/NefDecoder.cpp:707-792), Nikon's "RAW S" files: 12-bit       */
/*    Y/Y/Cb/Cr packets.  NefDecoder keeps its host work: the container and  */
/*    DecodeSNefUncompressed (:383-400), the white balance and its check     */
/*    (:671-687), inv_wb = int(1024.0F / wb) (:693-694), gammaCurve (:696-   */
/*    703) and the curve guard (:705), which always installs the DITHERING   */
/*    TableLookUp (its third argument is the literal false).                 */
/*    W = dim_x pixels; row y is exactly the bytes [3 W y, 3 W (y + 1)), and */
/*    holds 3 W 16-bit samples in the image (cpp 3).  Group g = 0 .. W/2 - 1 */
/*    is the bytes b0..b5 at 6 g, four 12-bit fields, LSB first:             */
/*      y1 = b0 | (b1 & 15) << 8, y2 = b1 >> 4 | b2 << 4,                    */
/*      cb = b3 | (b4 & 15) << 8, cr = b4 >> 4 | b5 << 4.                    */
/*    Pixel 1 of the group uses (y1, cb, cr), pixel 2 (y2, cb2, cr2) with    */
/*    cb2 = (float(cb of g + 1) + float(cb)) * 0.5F, cr2 likewise (exact in  */
/*    binary32), in the last group of a row cb2 = cb, cr2 = cr.  2048 comes  */
/*    off all four chroma values.  Per pixel, in binary64, every product and */
/*    every sum rounded on its own (no fused multiply-add), left to right:   */
/*      e0 = y + 1.370705 cr, e1 = (y - 0.337633 cb) - 0.698001 cr,          */
/*      e2 = y + 1.732446 cb; v_k = clampBits(int(e_k), 12) (truncation).    */
/*    Each v goes through setWithLookUp (RawImage.h:335-353): t = base +     */
/*    ((delta (r & 2047) + 1024) >> 12) mod 2^16 with base = table[2 v],     */
/*    delta = table[2 v + 1] (8192 entries read), then r = 15700 (r & 65535) */
/*    + (r >> 16) -- in the order of the six samples, so the step number of  */
/*    a sample is its index 6 g + k in the output row; r at the start of a   */
/*    row is b0 + (b1 << 8) + (b2 << 16) of the row's first three bytes (a   */
/*    seed of 0 stays 0).  Samples 1 and 4 (green) store t; samples 0 and 3  */
/*    clampBits((inv_wb_r t + 512) >> 10, 15), samples 2 and 5 the same with */
/*    inv_wb_b.  Nothing in the data can fail: there is no per-row status.   */
/*    The table is copied during the call (or at plan creation).             */
/*    rsx_nikon_snef_validate, in this order: desc NULL or table NULL ->     */
/*    RSX_ERR_INVALID_ARG; DecodeSNefUncompressed's checks (:389-394): cpp   */
/*    != 3, dim_x or dim_y <= 0, dim_x odd, dim_x > 3680, dim_y > 2456 (and  */
/*    pitch_bytes < 6 dim_x) -> RSX_ERR_INVALID_ARG; dim_x < 6 (:666-667,    */
/*    ThrowIOE) -> RSX_ERR_IO; an inv_wb outside 102 .. 32768 ->             */
/*    RSX_ERR_INVALID_ARG: the reference's check (:682-687) lets through     */
/*    float(13421568.0 / 429496627.0) = 0.03124953 <= wb <= 10.0F, and       */
/*    int(1024.0F / wb) is 102 = int(102.4F) at one end and 32768 =          */
/*    int(32768.492F) at the other; 32768 * 65535 + 512 = 2147451904 keeps   */
/*    inv_wb t + 512 inside int; in_bytes < 3 dim_x dim_y (input.peekData)   */
/*    -> RSX_ERR_IO.  Bytes behind 3 dim_x dim_y are not read; a job         */
/*    consumes exactly that many.  Pitch padding and everything outside the  */
/*    image are never written.                                               */
/* ------------------------------------------------------------------------ */
typedef struct rsx_nikon_snef_desc {
  int32_t inv_wb_r, inv_wb_b; /* int(1024.0F / wb), NefDecoder.cpp:693-694 */
  const uint16_t* table;      /* TableLookUp::tables, dither form: [2 v] base, [2 v + 1] delta;
                                 8192 entries read */
} rsx_nikon_snef_desc;

int rsx_nikon_snef_validate(const rsx_nikon_snef_desc* desc, const rsx_image* img,
                            size_t in_bytes);
int rsx_nikon_snef_decompress(rsx_ctx* ctx, const rsx_nikon_snef_desc* desc, const uint8_t* in,
                              size_t in_bytes, const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 3n. IiqDecoder::CorrectPhaseOneC: flat field, quadrant curves, defects    */
/*    replaces the pixel passes of PhaseOneFlatField (decoders/IiqDecoder    */
/*    .cpp:410-479) and CorrectQuadrantMultipliersCombined (:335-405) behind */
/*    PhaseOneDecompressor::decompress().  IiqDecoder keeps the parse of the */
/*    correction block (:280-325), the spline (Spline<>::calculateCurve, its */
/*    checks included) and mBadPixelPositions.  The image is uint16,         */
/*    cpp 1.  A flat field and the curves read and write only the pixel they */
/*    stand on, so a run of them, in file order, is ONE pass on the device:  */
/*    each pixel gets the whole run.  The sensor defects (entry 0x400) read  */
/*    neighbouring columns: such an op ends a run, runs as a launch over     */
/*    (record, row) of its own on the same stream, and the ops behind it are */
/*    the next run.                                                          */
/*    RSX_IIQ_OP_FLAT_FIELD: `payload` is the entry's bytes as they are in   */
/*    the file; nc = 2 (luma, entry 0x410) or 4 (`chroma`, entry 0x40b).     */
/*    head[0..7] = eight little-endian u16.  Any of head[2..5] zero: the op  */
/*    does nothing.  wide = ceil(head[2] / head[4]), high = ceil(head[3] /   */
/*    head[5]); behind the head high x wide x nc/2 u16 values v(y, x, c),    */
/*    num = v / 32768.0F.  mrow(x, c) = num at y = 0; at every y >= 1 the    */
/*    slope mrow(x, c + 1) = (num - mrow(x, c)) / head[5], then for the rows */
/*    head[1] + (y - 1) head[5] <= row < min(dim_y, head[1] + y head[5],     */
/*    head[1] + head[3] - head[5]): for x = 1 .. wide - 1 mult[c] =          */
/*    mrow(x - 1, c), step = (mrow(x, c) - mult[c]) / head[4], and for the   */
/*    columns head[0] + (x - 1) head[4] <= col < min(dim_x, head[0] + x      */
/*    head[4], head[0] + head[2] - head[4]): pixel = min(unsigned(float(     */
/*    pixel) * mult[c]), 65535) (truncation; a product below 0 gives 0),     */
/*    then mult[c] += step for every plane; after the row mrow(x, c) +=      */
/*    mrow(x, c + 1).  All of it in binary32, every operation rounded on its */
/*    own, the running sums as REPEATED additions (their drift feeds the     */
/*    next slope).  Luma: c = 0 at every pixel.  Chroma: c = cfa[(row mod    */
/*    cfa_w) + (col mod cfa_h) cfa_w] -- the reference's getColorAt(row,     */
/*    col), row passed as x -- 0 (red) uses plane 0, 2 (blue) plane 2, odd   */
/*    colours leave the pixel alone.                                         */
/*    RSX_IIQ_OP_QUADRANT_CURVES: `curves` = four curves of 65536 u16,       */
/*    [quadRow][quadCol]; quadRow = row >= split_row, quadCol = col >=       */
/*    split_col; diff = pixel < black_level ? pixel : uint16(black_level);   */
/*    pixel = uint16(curve[pixel - diff] + diff).                            */
/*    RSX_IIQ_OP_SENSOR_DEFECTS (correctSensorDefects, :499-576): `payload`  */
/*    / `payload_bytes` are the bytes of entry 0x400 as the file has them:   */
/*    8-byte records of little-endian u16 col, row, type and 2 ignored       */
/*    bytes.  Ops apply in list order: a defects op sees the image as the    */
/*    ops in front of it left it, the ops behind it see its result.  Records */
/*    apply in file order.  A record with col >= dim_x is skipped whatever   */
/*    its type; type 129 (a bad pixel) touches no pixel -- its position goes */
/*    to mBadPixelPositions, see rsx_iiq_defect_positions; any type other    */
/*    than 131 / 137 does nothing.  Type 131 / 137 (a bad column): for row   */
/*    in 2 .. dim_y - 3, colour = cfa[(col mod cfa_w) + (row mod cfa_h)      */
/*    cfa_w] -- getColorAt(col, row), NOT the transposed look-up of chroma.  */
/*    Green (1): val[0..3] = the pixels at (row - 1, col - 1), (row + 1,     */
/*    col - 1), (row - 1, col + 1), (row + 1, col + 1), sum their total,     */
/*    dev[i] = |4 val[i] - sum|; the FIRST largest dev is dropped (the       */
/*    comparison is a strict <, four equal values drop val[0]): pixel =      */
/*    (sum - val[max] + 1) / 3 in integers.  Any other colour: diags = the   */
/*    sum of the four pixels at (row +- 2, col +- 2), horiz = the sum of the */
/*    two at (row, col +- 2), pixel = lround(diags * 0.0732233 + horiz *     */
/*    0.3535534) in binary64, each operation rounded on its own (at most     */
/*    65535).  A column is written from other columns only, so the rows of a */
/*    record are independent and records whose columns differ by more than 2 */
/*    commute; records within 2 of each other (the same column twice         */
/*    included) take effect in file order: the host sorts the records into   */
/*    levels, one launch a level -- a list of columns far apart is a single  */
/*    launch.                                                                */
/*    rsx_iiq_correct_validate, in this order: corr or img NULL, cpp != 1,   */
/*    dim_x or dim_y <= 0, pitch_bytes < 2 dim_x -> RSX_ERR_INVALID_ARG;     */
/*    n_ops outside 0..16, an unknown kind (2 is not used and stays unknown),*/
/*    a NULL payload of a flat field or NULL curves ->                       */
/*    RSX_ERR_INVALID_ARG; then per op in list order: a payload shorter than */
/*    16 bytes, or shorter than 16 + 2 high wide nc/2 when no head field     */
/*    2..5 is zero -> RSX_ERR_IO (the reference throws half-way through the  */
/*    image and the file fails); chroma with cfa_w cfa_h == 0 or > 64 ->     */
/*    RSX_ERR_INVALID_ARG ("No CFA size set"); chroma with an even colour    */
/*    other than 0 or 2 in the CFA -> RSX_ERR_UNSUPPORTED (the reference     */
/*    indexes mult[4..] outside its array); split_row > dim_y or split_col   */
/*    > dim_x -> RSX_ERR_INVALID_ARG; a flat field whose row table (touched  */
/*    rows x cells in reach of the image x nc/2 floats) exceeds 2^26 floats  */
/*    (256 MiB; 1 x 1 cells over a full 11976 x 8854 frame would take 848    */
/*    MiB, cells of 4 x 4 and up fit; cells wider than 32 columns keep a     */
/*    start value every 32 columns on top, rows x width / 32 x nc/2 floats)  */
/*    -> RSX_ERR_UNSUPPORTED.  Behind all of these, the defects ops: a       */
/*    second one in a list -> RSX_ERR_INVALID_ARG (the reference throws      */
/*    "Second sensor defects entry seen"); payload NULL with payload_bytes > */
/*    0 -> RSX_ERR_INVALID_ARG (payload_bytes == 0: the op does nothing);    */
/*    payload_bytes no multiple of 8 -> RSX_ERR_IO (the reference's reader   */
/*    throws half-way and the file fails); then the records in file order,   */
/*    the first offender decides -- only records of type 131 / 137 with col  */
/*    < dim_x count, and only when dim_y >= 5 (otherwise the loop has no row */
/*    and nothing is read): cfa_w cfa_h == 0 or > 64 -> RSX_ERR_INVALID_ARG  */
/*    ("No CFA size set"); col < 2 or col > dim_x - 3 -> RSX_ERR_UNSUPPORTED */
/*    (the reference reads outside the row there; the host path keeps what-  */
/*    ever it does); more than 4096 such records -> RSX_ERR_UNSUPPORTED.     */
/*    On any status but RSX_OK the image is untouched.  n_ops == 0 is        */
/*    RSX_OK and writes nothing; pixels outside every op's area and pitch    */
/*    padding are never written.  Payloads and curves are copied during the  */
/*    call (or at plan creation).                                            */
/*    rsx_iiq_correct works in place; img->data may be a host pointer (the   */
/*    image goes up, is corrected and comes back) or a device pointer (the   */
/*    call returns when the pass is done).                                   */
/*    rsx_phase_one_decompress_corrected = rsx_phase_one_decompress, the     */
/*    list applied to the decoded image on the device, ONE download.  A      */
/*    failing strip or a refused list leaves the caller's image untouched.   */
/*    rsx_iiq_defect_positions (host only): the type-129 records of an entry */
/*    0x400 with col < dim_x, in file order, as (row << 16) + col -- what    */
/*    handleBadPixel inserts into mBadPixelPositions; row is not checked, as */
/*    in the reference.  Up to `cap` go to `out` (may be NULL with cap 0),   */
/*    *n is the full count even past cap.  payload_bytes no multiple of 8 -> */
/*    RSX_ERR_IO; payload NULL with payload_bytes > 0, out NULL with cap >   */
/*    0, n NULL -> RSX_ERR_INVALID_ARG.                                      */
/*    rsx_phase_one_decompress_fixed = rsx_phase_one_decompress_corrected,   */
/*    then the stage of section 5 on the positions of the list's defects op  */
/*    (is_cfa as img has it), in front of the ONE download.  map_out (may be */
/*    NULL; createBadPixelMap's pitch as map_pitch, 0 allowed without        */
/*    map_out) receives the map, result (may be NULL) the counts.  With no   */
/*    positions (no defects op included) there is no map: map_made = 0,      */
/*    map_out untouched, and the call is the _corrected call.  Statuses as   */
/*    the _corrected call, then the stage's own (section 5: an image         */
/*    dimension past 65536, a wrong map_pitch, a position at row >= dim_y);  */
/*    on anything but RSX_OK the caller's image and map_out are untouched.   */
/* ------------------------------------------------------------------------ */
#define RSX_IIQ_MAX_OPS 16
typedef enum rsx_iiq_op_kind {
  RSX_IIQ_OP_FLAT_FIELD = 0,
  RSX_IIQ_OP_QUADRANT_CURVES = 1,
  /* (2 is not used: rsx_iiq_correct_validate refuses it as an unknown kind) */
  RSX_IIQ_OP_SENSOR_DEFECTS = 3
} rsx_iiq_op_kind;

typedef struct rsx_iiq_op {
  int32_t kind;           /* rsx_iiq_op_kind */
  int32_t chroma;         /* flat field: 0 luma (0x410), 1 chroma (0x40b) */
  const uint8_t* payload; /* flat field: the entry's bytes, head included; defects: entry 0x400 */
  uint32_t payload_bytes;
  uint32_t black_level;   /* quadrant curves: IiqDecoder::black_level */
  const uint16_t* curves; /* quadrant curves: 4 x 65536, [quadRow][quadCol] */
  uint32_t split_row, split_col;
} rsx_iiq_op;

typedef struct rsx_iiq_corr {
  int32_t n_ops;
  int32_t cfa_w, cfa_h; /* mRaw->cfa.getSize(); 0 x 0: none */
  uint8_t cfa[64];      /* CFAColor values, cfa[x + y cfa_w] */
  rsx_iiq_op ops[RSX_IIQ_MAX_OPS];
} rsx_iiq_corr;

int rsx_iiq_correct_validate(const rsx_iiq_corr* corr, const rsx_image* img);
int rsx_iiq_correct(rsx_ctx* ctx, const rsx_iiq_corr* corr, const rsx_image* img);
int rsx_phase_one_decompress_corrected(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes,
                                       int n_strips, const rsx_phase_one_strip* strips,
                                       const rsx_iiq_corr* corr, const rsx_image* img,
                                       int32_t* strip_status);
int rsx_iiq_defect_positions(const uint8_t* payload, uint32_t payload_bytes, int32_t dim_x,
                             uint32_t* out, uint32_t cap, uint32_t* n);
struct rsx_bad_pixels_result; /* section 5 */
int rsx_phase_one_decompress_fixed(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes, int n_strips,
                                    const rsx_phase_one_strip* strips, const rsx_iiq_corr* corr,
                                    const rsx_image* img, int32_t* strip_status, uint8_t* map_out,
                                    uint32_t map_pitch, struct rsx_bad_pixels_result* result);

/* ------------------------------------------------------------------------ */
/* 3u. FujiDecompressor (compressed RAF)                                     */
/*    replaces FujiDecompressor::decompress()                                */
/*    (decompressors/FujiDecompressor.cpp:901-908 -> decompressThread        */
/*    :805-826 -> fuji_decode_strip :734-779 per strip).  The constructor    */
/*    keeps its host work, the CFA checks included (:864-879).               */
/*    rsx_fuji_parse = what the constructor does with the stream (:850-899): */
/*    the big-endian 16-byte header (u16 signature, u8 version, u8 raw_type, */
/*    u8 raw_bits, u16 raw_height, u16 raw_rounded_width, u16 raw_width,     */
/*    u16 block_size, u8 blocks_in_row, u16 total_lines), blocks_in_row u32  */
/*    sizes, 0x10 - (4 blocks_in_row & 0xC) bytes of padding where           */
/*    4 blocks_in_row & 0xC is not zero, then the strips one after another;  */
/*    every read past the end -> RSX_ERR_IO.  A header that FujiHeader::     */
/*    operator bool refuses leaves n_strips 0 and RSX_OK: the refusal is     */
/*    rsx_fuji_validate's, and no size is read.                              */
/*    rsx_fuji_validate = the constructor's checks in its order: cpp 1 (an   */
/*    rsx_image is UINT16), FujiHeader::operator bool (:919-937), dim ==     */
/*    (raw_width, raw_height) (and pitch_bytes >= 2 dim_x) ->                */
/*    RSX_ERR_INVALID_ARG; raw_bits 12 -> RSX_ERR_UNSUPPORTED (:859-862,     */
/*    the reference throws); fuji_block_checks (:191-194) and n_strips !=    */
/*    blocks_in_row -> RSX_ERR_INVALID_ARG.  A strip that does not lie in    */
/*    the `in_bytes` of a call (getStream) -> RSX_ERR_IO from the call.      */
/*    A frame is blocks_in_row strips of 768 columns, each one               */
/*    BitStreamerMSB over exactly its own bytes (bytes behind it read as     */
/*    zero), 18 line buffers of line_width + 2 samples (512 for raw_type 16, */
/*    X-Trans; 384 for raw_type 0, Bayer) and two sets of three tables of 41 */
/*    {value1, value2} pairs starting at {1 << (raw_bits - 6), 1}.  Every    */
/*    strip decodes line_width samples a line; the copy-out of the last one  */
/*    is raw_width - 768 n columns wide.                                     */
/*    Per-strip statuses, the first exception of the strip in stream order:  */
/*      RSX_ERR_IO              strip shorter than 4 bytes ("Bit stream size */
/*                              is smaller than MaxProcessBytes")            */
/*      RSX_ERR_INPUT_OVERFLOW  a refill more than 8 bytes past the strip    */
/*                              (BitStreamer.h:100-132).  Every request is   */
/*                              fill(32), one per batch of the zero count    */
/*                              and one in front of the code bits: with c    */
/*                              bits consumed and k words loaded the cache   */
/*                              holds 32 k - c bits, a fill loads iff that   */
/*                              is below 32, and k = ceil(c / 32) + 1 behind */
/*                              it.  The load of word k throws iff           */
/*                              4 k > size + 8, so a fill at c fails iff     */
/*                              4 ceil(c / 32) > size + 8                    */
/*      RSX_ERR_VALUE_RANGE     code < 0 || code >= total_values (:467)      */
/*    The reference collects the strips' errors and throws if there is one;  */
/*    the call returns the status of the lowest-numbered failing strip, and  */
/*    through host pointers leaves the caller's image untouched then.  The   */
/*    other strips are decoded.  `in` and `img->data` are both host or both  */
/*    device pointers.  `strip_status` (may be NULL) gets n_strips statuses. */
/* ------------------------------------------------------------------------ */
#define RSX_FUJI_MAX_STRIPS 16
typedef struct rsx_fuji_desc {
  int32_t signature; /* 0x4953 */
  int32_t version;   /* 1 */
  int32_t raw_type;  /* 16 X-Trans, 0 Bayer */
  int32_t raw_bits;
  int32_t raw_height;
  int32_t raw_rounded_width;
  int32_t raw_width;
  int32_t block_size;
  int32_t blocks_in_row;
  int32_t total_lines;
  int32_t n_strips;
  int32_t reserved;
  uint64_t strip_offset[RSX_FUJI_MAX_STRIPS]; /* into `in` */
  uint32_t strip_bytes[RSX_FUJI_MAX_STRIPS];
} rsx_fuji_desc;

int rsx_fuji_parse(const uint8_t* in, size_t in_bytes, rsx_fuji_desc* desc);
int rsx_fuji_validate(const rsx_fuji_desc* desc, const rsx_image* img);
int rsx_fuji_decompress(rsx_ctx* ctx, const rsx_fuji_desc* desc, const uint8_t* in,
                        size_t in_bytes, const rsx_image* img, int32_t* strip_status);

/* ------------------------------------------------------------------------ */
/* 3v. OlympusDecompressor (compressed ORF)                                  */
/*    replaces OlympusDecompressor::decompress()                             */
/*    (decompressors/OlympusDecompressor.cpp:229-231 -> :204-214, per row    */
/*    decompressRow :183-202, per pixel getDiff :61-97 and getPred           */
/*    :130-164); OrfDecoder::decodeUncompressed is rsx_unpack_* already.     */
/*    rsx_olympus_validate = the constructor's checks in its order           */
/*    (:218-227): cpp 1 (an rsx_image is UINT16); dim_x and dim_y positive   */
/*    and even, dim_x <= 10400, dim_y <= 7792; and pitch_bytes >= 2 dim_x    */
/*    -> RSX_ERR_INVALID_ARG.  Then what the reader refuses before the first */
/*    bit: in_bytes < 7 (skipBytes(7), :209) and in_bytes - 7 < 4 ("Bit      */
/*    stream size is smaller than MaxProcessBytes", BitStreamer.h:58-59)     */
/*    -> RSX_ERR_IO.                                                         */
/*    `in` is the stream as OrfDecoder hands it over, the 7 bytes in front   */
/*    included.  Behind them one BitStreamerMSB runs over all rows with no   */
/*    alignment or marker between them; each row starts two difference       */
/*    decoders (one a column parity) at carry {0, 0, 0}.  Every byte string  */
/*    is a stream: the only failures are the reader's.                       */
/*    Statuses of a decode:                                                  */
/*      RSX_ERR_INVALID_ARG     the constructor's refusals, the pitch, an    */
/*                              odd pitch or image offset, host and device   */
/*                              pointers mixed                               */
/*      RSX_ERR_IO              fewer than 11 bytes                          */
/*      RSX_ERR_INPUT_OVERFLOW  a refill more than 8 bytes past the end      */
/*                              (BitStreamer.h:100-132).  Every request is   */
/*                              fill(32), one in front of every symbol, and  */
/*                              a symbol takes at most 31 bits: as in 3u, a  */
/*                              fill with c bits consumed fails iff          */
/*                              4 ceil(c / 32) > size + 8, size =            */
/*                              in_bytes - 7.  Bytes past the end read as    */
/*                              zero until then.                             */
/*    `in` and `img->data` are both host or both device pointers.  Through   */
/*    host pointers a failing call leaves the caller's image untouched;      */
/*    through device pointers the image behind a failure is unspecified      */
/*    (the walk writes differences into it).                                 */
/* ------------------------------------------------------------------------ */
int rsx_olympus_validate(size_t in_bytes, const rsx_image* img);
int rsx_olympus_decompress(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes,
                           const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 3w. KodakDecompressor (Kodak DCR, TIFF compression 65000)                 */
/*    replaces KodakDecompressor::decompress()                               */
/*    (decompressors/KodakDecompressor.cpp:120-150, per segment              */
/*    decodeSegment :67-118), reached from DcrDecoder::decodeRawInternal     */
/*    (decoders/DcrDecoder.cpp:58-120), with setWithLookUp                   */
/*    (common/RawImage.h:335-353) and the curve guard (:355-383) that        */
/*    installs mRaw->table before the call.                                  */
/*    Rows top to bottom, each cut into segments of len = min(256, dim_x -   */
/*    col) pixels: n = dim_x / 256 full ones, then a tail of t = dim_x % 256 */
/*    if t != 0.  A segment is, in order:                                    */
/*      len / 2 bytes of lengths: pixel 2k the low nibble of byte k, pixel   */
/*        2k + 1 the high nibble (0..15);                                    */
/*      the bit area, big-endian 16-bit units, each consumed from its least  */
/*        significant bit upward: one unit up front if (len & 7) == 4        */
/*        (init = 16 bits, else 0), then two units (4 bytes) whenever the    */
/*        bits held are fewer than the next pixel's length.                  */
/*    With cum(i) the sum of the lengths of pixels 0..i-1, pixel i's field   */
/*    is bits [cum(i), cum(i) + len_i) of the units' concatenation (bit p:   */
/*    bit p % 16 of the unit at byte 2 (p / 16)), there are                  */
/*    r = ceil(max(0, cum(len) - init) / 32) 4-byte reads, and the segment   */
/*    takes len / 2 + init / 8 + 4 r bytes: always an even number, so every  */
/*    segment starts at an even offset of the stream.                        */
/*    diff = 0 for length 0, else the JPEG extend of the field; pred[2] =    */
/*    {0, 0} at every segment's start, pred[i & 1] += diff, and value =      */
/*    pred[i & 1] must lie in 0 .. 2^bps - 1 ("Value out of bounds").  The   */
/*    value stored is setWithLookUp(value) with the table `desc` describes:  */
/*      RSX_KODAK_TABLE_NONE    no table (uncorrectedRawValues): the value   */
/*      RSX_KODAK_TABLE_PLAIN   table[value] (2^bps entries read)            */
/*      RSX_KODAK_TABLE_DITHER  table[2 value] (2^(bps + 1) entries read):   */
/*                              the generator starts at 0 for the whole      */
/*                              image and 15700 * 0 + 0 is 0, so the delta   */
/*                              never contributes ((delta * 0 + 1024) >> 12  */
/*                              is 0)                                        */
/*    The table is copied during the call (or at plan creation).             */
/*    rsx_kodak_validate: desc or img NULL, an unknown table_mode, or a NULL */
/*    table with a mode other than NONE -> RSX_ERR_INVALID_ARG; then the     */
/*    constructor's checks in its order (:46-65): cpp 1; dim positive,       */
/*    dim_x % 4 == 0, dim_x <= 4516, dim_y <= 3012; bps 10 or 12 (and        */
/*    pitch_bytes >= 2 dim_x) -> RSX_ERR_INVALID_ARG; in_bytes <             */
/*    dim_x dim_y / 2 (input.check) -> RSX_ERR_IO.                           */
/*    `in` is what DcrDecoder hands over: the rest of the file from the      */
/*    strip's offset, so there usually are trailing bytes.  An image cannot  */
/*    consume more than dim_y times the sum over a row's segments of         */
/*    len / 2 + 2 + 4 ceil(15 len / 32) bytes; what lies behind is not read  */
/*    (and not uploaded by a host-pointer call).                             */
/*    Statuses of a decode, as the reference reaches them in decode order    */
/*    (the first failing segment decides; inside a segment the read comes    */
/*    first, decodeSegment reads all of it before the values are summed):    */
/*      RSX_ERR_IO           a segment reads past in_bytes (getByte)         */
/*      RSX_ERR_VALUE_RANGE  a value below 0 or above 2^bps - 1              */
/*    `in` and `img->data` are both host or both device pointers.  Through   */
/*    host pointers a failing call leaves the caller's image untouched;      */
/*    through device pointers the image behind a failure is unspecified      */
/*    (segments are decoded side by side), its pitch padding untouched.      */
/* ------------------------------------------------------------------------ */
enum {
  RSX_KODAK_TABLE_NONE = 0,
  RSX_KODAK_TABLE_PLAIN = 1,
  RSX_KODAK_TABLE_DITHER = 2
};

typedef struct rsx_kodak_desc {
  int32_t bps;           /* 10 or 12 */
  int32_t table_mode;    /* RSX_KODAK_TABLE_* */
  const uint16_t* table; /* TableLookUp::tables: 2^bps (PLAIN) / 2^(bps + 1) (DITHER) entries */
} rsx_kodak_desc;

int rsx_kodak_validate(const rsx_kodak_desc* desc, const rsx_image* img, size_t in_bytes);
int rsx_kodak_decompress(rsx_ctx* ctx, const rsx_kodak_desc* desc, const uint8_t* in,
                         size_t in_bytes, const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 3x. CrwDecompressor (Canon CRW: EOS D30 / D60 / 10D / 300D, PowerShot G, S) */
/*    replaces CrwDecompressor::decompress()                                 */
/*    (decompressors/CrwDecompressor.cpp:210-286, per block decodeBlock      */
/*    :167-207), reached from CrwDecoder::decodeRawInternal                  */
/*    (decoders/CrwDecoder.cpp:71-123).                                      */
/*    `in` is the scan: Huffman-coded and JPEG-stuffed (FF 00 is a data FF,  */
/*    FF xx with xx != 00 ends the stream), one chain for the whole frame.   */
/*    It holds dim_x dim_y / 64 blocks of 64 differences.  A symbol is a     */
/*    code of the table number's first tree (coefficient 0) or second tree   */
/*    (behind it) whose value is run << 4 | len: 00 behind coefficient 0     */
/*    ends the block, ff moves on by one, else the index moves on by run,    */
/*    len == 0 moves on by one more, and otherwise len bits follow (consumed */
/*    even when the run has passed coefficient 63) and are the JPEG extend   */
/*    of coefficient i.  Coefficient 0 carries a running sum over all blocks */
/*    of the frame.  Pixel k of the frame (row-major) adds difference k to   */
/*    one of two running sums, by the parity of k & 63 -- which is the       */
/*    parity of the column, dim_x being even -- both 512 at every row's      */
/*    start; a sum outside 0..1023 is "Error decompressing".  With low bits, */
/*    a pixel becomes pixel << 2 | two bits of `low` (one byte per four      */
/*    pixels, the first pixel in bits 0..1), and where dim_x == 2672 a       */
/*    result below 512 gets + 2.                                             */
/*    The refill rule as a closed form of consumed bits: the reader calls    */
/*    fill(32) in front of every symbol, so in front of a symbol that starts */
/*    at consumed bit c it has fetched 4 (ceil(c / 32) + 1) data bytes, and  */
/*    fill k (from 0) is taken at the first symbol start c > 32 (k - 1).     */
/*    Behind the data the reader supplies zeros.  Without a marker, with N   */
/*    data bytes in in_bytes raw bytes that end at R (in_bytes, or           */
/*    in_bytes + 1 when the last byte is FF), the first symbol start         */
/*    c > 32 floor((in_bytes + 16 + N - R) / 4) is the overflow read.  A     */
/*    marker behind M data bytes is met by fill floor(M / 4), at symbol      */
/*    start cm; it leaves 64 bits in the cache and four more fills pass, so  */
/*    the first symbol start c > cm + 160 is the overflow read.  A frame     */
/*    whose last block ends in front of that decodes.                        */
/*    rsx_crw_validate: desc or img NULL -> RSX_ERR_INVALID_ARG; then the    */
/*    constructor's checks (:46-72, :87-89): cpp 1; dim positive, dim_x % 4  */
/*    == 0, dim_x <= 4104, dim_y <= 3048, dim_x dim_y % 64 == 0; dec_table   */
/*    <= 2; with has_lowbits, low_bytes >= dim_x dim_y / 4 (and pitch_bytes  */
/*    >= 2 dim_x) -> RSX_ERR_INVALID_ARG; in_bytes < 8 (the reader's         */
/*    MaxProcessBytes) -> RSX_ERR_IO.                                        */
/*    Statuses of a decode: the first failure in the reference's order,      */
/*    which is block b's parse, then block b's 64 pixels, then block b + 1:  */
/*      RSX_ERR_BAD_HUFFMAN_CODE  no code of the tree matches                */
/*      RSX_ERR_INPUT_OVERFLOW    the overflow read above                    */
/*      RSX_ERR_VALUE_RANGE       a pixel outside 0..1023                    */
/*    `in`, `low` (NULL without low bits) and `img->data` are all host or    */
/*    all device pointers; pitch_bytes is even.  Only the first              */
/*    min(in_bytes, 496 dim_x dim_y / 64 + 2) bytes of `in` and the first    */
/*    dim_x dim_y / 4 of `low` are read.  Bytes of the image outside its     */
/*    rows are untouched.  Through host pointers a failing call leaves the   */
/*    caller's image untouched; through device pointers the image behind a   */
/*    failure is unspecified.                                                */
/* ------------------------------------------------------------------------ */
typedef struct rsx_crw_desc {
  uint32_t dec_table;   /* 0..2: which pair of trees */
  uint32_t has_lowbits; /* != 0: the two low bits of every pixel come from `low` */
} rsx_crw_desc;

int rsx_crw_validate(const rsx_crw_desc* desc, const rsx_image* img, size_t in_bytes,
                     size_t low_bytes);
int rsx_crw_decompress(rsx_ctx* ctx, const rsx_crw_desc* desc, const uint8_t* in, size_t in_bytes,
                       const uint8_t* low, size_t low_bytes, const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 3y. RafDecoder::applyCorrections: the 45 degree rotation of SuperCCD      */
/*    frames (decoders/RafDecoder.cpp:228-270; the cameras with the          */
/*    fuji_rotate hint)                                                      */
/*    With W x H = new_size (size_x, size_y), (cx, cy) = crop_offset and     */
/*    R = rotatedsize, sample src(cy + y, cx + x) of the uncropped uint16    */
/*    image goes to dst(h, w):                                               */
/*      normal  R = W + H / 2  h = W - 1 - x + (y >> 1)                      */
/*                             w = ((y + 1) >> 1) + x                        */
/*      alt     R = H + W / 2  h = R - (H + 1 - y + (x >> 1))                */
/*                             w = ((x + 1) >> 1) + y                        */
/*    dst is R wide and R - 1 tall; every sample nothing lands on is 0       */
/*    (clearArea).  metadata.fujiRotationPos is W - 1 (normal) or W / 2 - 1  */
/*    (alt).  Bytes of dst's pitch beyond R samples are not written.         */
/*    rsx_raf_rotate_validate, in this order: desc, src or dst NULL; cpp    */
/*    != 1 on either image; a dimension <= 0; a pitch below 2 dim_x, or odd; */
/*    size_x < 1 or size_y < 1; a negative crop offset; crop + size beyond   */
/*    src (the reference would read outside its image); R < 2 or R > 65535   */
/*    (RawImage::createData throws); dst other than R x (R - 1); src and dst */
/*    (both with data) overlapping; the normal layout with odd size_y (the   */
/*    reference throws "Trying to write out of bounds": (y = H - 1, x = 0)   */
/*    lands on row R - 1) -> RSX_ERR_INVALID_ARG.  Then alt_layout with odd  */
/*    size_x -> RSX_ERR_UNSUPPORTED: (y = 0, x = W - 1) lands on row -1,     */
/*    which the reference's signed `h < dim.y` does not catch.               */
/*    rsx_raf_rotate_geometry applies the checks that need no image, in the */
/*    same order, and gives dst's size and fujiRotationPos (outputs may be   */
/*    NULL; untouched on a failure).                                         */
/*    rsx_raf_rotate: src->data and dst->data are both host pointers (the   */
/*    rows of the crop go up, the rotated image comes back) or both device   */
/*    pointers (the call returns when the pass is done).  One launch writes  */
/*    every sample of dst.  On any status but RSX_OK dst is untouched.       */
/* ------------------------------------------------------------------------ */
typedef struct rsx_raf_rotate_desc {
  int32_t crop_x, crop_y; /* crop_offset */
  int32_t size_x, size_y; /* new_size */
  int32_t alt_layout;
  int32_t reserved;
} rsx_raf_rotate_desc;

int rsx_raf_rotate_geometry(const rsx_raf_rotate_desc* desc, int32_t* out_dim_x,
                             int32_t* out_dim_y, int32_t* rotation_pos);
int rsx_raf_rotate_validate(const rsx_raf_rotate_desc* desc, const rsx_image* src,
                             const rsx_image* dst);
int rsx_raf_rotate(rsx_ctx* ctx, const rsx_raf_rotate_desc* desc, const rsx_image* src,
                    const rsx_image* dst);

/* ------------------------------------------------------------------------ */
/* 3z. ArwDecoder::SonyDecrypt and ArwDecoder::decodeSRF (Sony SRF, DSC-F828) */
/*    (decoders/ArwDecoder.cpp:524-560 and :70-118)                          */
/*    The pad from `key`, uint32 wrapping: pad[p] = key = key 48828125 + 1   */
/*    for p = 0..3; pad[3] = pad[3] << 1 | (pad[0] ^ pad[2]) >> 31; pad[p] = */
/*    (pad[p-4] ^ pad[p-2]) << 1 | (pad[p-3] ^ pad[p-1]) >> 31 for p =       */
/*    4..126; then every entry byte-swapped.  With w[0..126] those values,   */
/*    w[n] = w[n - 127] ^ w[n - 63] for n >= 127, and output word i is input */
/*    word i (4 bytes, as a little-endian uint32) ^ w[127 + i].              */
/*    rsx_sony_decrypt runs that over n_words words: `in` and `out` are both */
/*    host or both device pointers, of any alignment; in == out is allowed,  */
/*    any other overlap is not; n_words == 0 is RSX_OK and does nothing;     */
/*    ctx NULL, or in / out NULL with n_words > 0 -> RSX_ERR_INVALID_ARG;    */
/*    n_words >= 2^32 -> RSX_ERR_UNSUPPORTED.                                */
/*    rsx_sony_srf_decompress is decodeSRF behind its key derivation (which  */
/*    stays with the caller: the byte at 200896, the 40-byte head at 164600  */
/*    through the same generator, four bytes of it): `in` is the image data  */
/*    at file offset 862144, `key` the final key.  2 dim_x dim_y bytes are   */
/*    decrypted and read as 16-bit big-endian rows of pitch 2 dim_x, in one  */
/*    pass over the bytes: pix(2j) = b0 << 8 | b1, pix(2j + 1) = b2 << 8 |   */
/*    b3 of decrypted word j, pixels counted along the rows.                 */
/*    rsx_sony_srf_validate, in this order: img NULL; cpp != 1; dimensions   */
/*    outside 1..3360 x 1..2460; a pitch below 2 dim_x, or odd ->            */
/*    RSX_ERR_INVALID_ARG; in_bytes < 2 dim_x dim_y (getSubView) ->          */
/*    RSX_ERR_IO; dim_x dim_y odd -> RSX_ERR_UNSUPPORTED (len / 4 drops two  */
/*    bytes and SonyDecrypt's size invariants do not hold).                  */
/*    `in` and `img->data` are both host or both device pointers.  On any    */
/*    status but RSX_OK the image is untouched; bytes of its pitch beyond    */
/*    dim_x samples are never written.                                       */
/* ------------------------------------------------------------------------ */
int rsx_sony_decrypt(rsx_ctx* ctx, const uint8_t* in, uint8_t* out, size_t n_words, uint32_t key);
int rsx_sony_srf_validate(size_t in_bytes, const rsx_image* img);
int rsx_sony_srf_decompress(rsx_ctx* ctx, const uint8_t* in, size_t in_bytes, uint32_t key,
                            const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 4. AbstractDngDecompressor tile fan-out                                   */
/*    replaces AbstractDngDecompressor::decompress()                         */
/*    (AbstractDngDecompressor.h:141, .cpp:240-252) for compression 1        */
/*    (decompressThread<1> .cpp:54-110: per-tile UncompressedDecompressor)   */
/*    and compression 7 (decompressThread<7> .cpp:112-131: per-tile          */
/*    LJpegDecoder; the host keeps parsing each tile's JPEG headers and      */
/*    hands us one rsx_ljpeg_desc per tile).  All tiles are decoded by ONE   */
/*    batched launch sequence instead of one OpenMP thread per tile.         */
/*    Per-tile failures are reported in tile_status[] (the reference appends */
/*    them to the ErrorLog, .cpp:122-129); the call returns                  */
/*    RSX_ERR_TILE_ERRORS if any tile failed (.cpp:247-251).                 */
/* ------------------------------------------------------------------------ */
typedef struct rsx_dng_ljpeg_tile {
  rsx_ljpeg_desc desc;
  const uint8_t* in; /* entropy-coded data of this tile */
  size_t in_bytes;
} rsx_dng_ljpeg_tile;

int rsx_dng_decompress_ljpeg(rsx_ctx* ctx, int n_tiles,
                             const rsx_dng_ljpeg_tile* tiles,
                             const rsx_image* img, int32_t* tile_status,
                             uint32_t* tile_consumed);

typedef struct rsx_dng_unpack_tile {
  rsx_unpack_desc desc;
  const uint8_t* in;
  size_t in_bytes;
} rsx_dng_unpack_tile;

int rsx_dng_decompress_uncompressed(rsx_ctx* ctx, int n_tiles,
                                    const rsx_dng_unpack_tile* tiles,
                                    const rsx_image* img,
                                    int32_t* tile_status);

/* ------------------------------------------------------------------------ */
/* 4b. AbstractDngDecompressor, compression 8: deflate + floating-point      */
/*    predictor (decompressThread<8>, AbstractDngDecompressor.cpp:134-155 -> */
/*    DeflateDecompressor, decompressors/DeflateDecompressor.cpp:49-176).    */
/*    All sizes are in SAMPLES: tile_w x tile_h = maxDim (cpp * tileW,       */
/*    tileH), width x height = dim (cpp * e.width, e.height), off_x, off_y = */
/*    off (cpp * e.offX, e.offY); cpp is the image's.  The image holds       */
/*    4-byte samples (RawImageType::F32).                                    */
/*    Per tile: predFactor = 1 / 2 / 4 for predictor 3 / 34894 / 34895,      */
/*    times cpp; bytesps = bps / 8; dstLen = bytesps * tile_w * tile_h.      */
/*    zlib's uncompress(buf, &dstLen, in, in_bytes): the zlib wrapper (CMF,  */
/*    FLG), the deflate blocks, the Adler-32; bytes behind the stream are    */
/*    ignored.  Then for every row below `height`, over rows of bytesps *    */
/*    tile_w bytes: b[col] += b[col - predFactor] mod 256 from predFactor to */
/*    the end of the row (across the byte planes); sample col = the bytes    */
/*    b[col + c * tile_w], c = 0 .. bytesps - 1, most significant first;     */
/*    binary16 and binary24 (1 + 7 + 16) widened as                          */
/*    extendBinaryFloatingPoint does, binary32 as it is; the first `width`   */
/*    samples go to out(off_y + row, off_x + col).  Nothing else of the      */
/*    image is written, its pitch padding included.                          */
/*    rsx_dng_deflate_validate, in this order: bps not 16 / 24 / 32;         */
/*    predictor not 3 / 34894 / 34895; an image that cannot hold 4-byte      */
/*    samples (cpp outside 1..4, no pixels, pitch_bytes no multiple of 4);   */
/*    an empty tile or window, width > tile_w, height > tile_h; the window   */
/*    outside the image; pitch_bytes < 4 cpp dim_x -> RSX_ERR_INVALID_ARG;   */
/*    in_bytes or dstLen >= 4 GiB -> RSX_ERR_UNSUPPORTED.                    */
/*    Per-tile status:                                                       */
/*      RSX_OK               libz answers Z_OK and gave exactly dstLen bytes */
/*                           (empty blocks behind a full output included)    */
/*      RSX_ERR_UNSUPPORTED  Z_OK with fewer bytes: the reference then reads */
/*                           indeterminate bytes of a reused buffer -- the   */
/*                           CPU gets the tile                               */
/*      RSX_ERR_IO           everything libz rejects ("failed to uncompress  */
/*                           tile"): a byte too many, a wrong Adler-32,      */
/*                           FDICT, CM != 8, a window above 15, a bad        */
/*                           FCHECK, BTYPE 3, LEN != ~NLEN, code length sets */
/*                           inflate_table rejects, a missing end-of-block   */
/*                           code, HLIT > 286, HDIST > 30, a bad repeat,     */
/*                           codes 286 / 287 / distance 30 / 31, a distance  */
/*                           before the output's start, truncation anywhere  */
/*    A tile that is not RSX_OK writes NOTHING into the image; the others    */
/*    are written.  The call returns RSX_ERR_TILE_ERRORS if any tile failed. */
/*    One upload of the packed tile bytes, one launch sequence, one download;*/
/*    one host call in rsx_ctx_host_calls.                                   */
/* ------------------------------------------------------------------------ */
typedef struct rsx_dng_deflate_desc {
  int32_t bps;       /* 16, 24 or 32 */
  int32_t predictor; /* 3, 34894 or 34895 */
} rsx_dng_deflate_desc;

typedef struct rsx_dng_deflate_tile {
  const uint8_t* in; /* the tile's zlib stream */
  size_t in_bytes;
  uint32_t tile_w, tile_h;               /* maxDim, samples */
  uint32_t off_x, off_y, width, height;  /* off, dim, samples */
} rsx_dng_deflate_tile;

int rsx_dng_deflate_validate(const rsx_dng_deflate_desc* desc, const rsx_dng_deflate_tile* tile,
                             const rsx_image* img);
int rsx_dng_decompress_deflate(rsx_ctx* ctx, const rsx_dng_deflate_desc* desc, int n_tiles,
                               const rsx_dng_deflate_tile* tiles, const rsx_image* img,
                               int32_t* tile_status);

/* ------------------------------------------------------------------------ */
/* 4c. AbstractDngDecompressor, compression 9: GoPro VC-5                    */
/*    replaces VC5Decompressor::decode (decompressThread<9>,                 */
/*    AbstractDngDecompressor.cpp:161-179 -> decompressors/VC5Decompressor   */
/*    .cpp).  The constructor keeps its host work: the checks of :384-424    */
/*    and the tag parse (parseVC5, parseLargeCodeblock); the caller hands    */
/*    over what the parse found, the code book and the log curve.            */
/*    The image is W x H 16-bit samples, cpp 1; four channels of ceil(W/2) x */
/*    ceil(H/2), each three wavelet levels deep: level k = 1..3 has bands of */
/*    w_k x h_k coefficients, w_k = ceil(w_(k-1) / 2), w_0 = ceil(W / 2).    */
/*    bands[c][s] is subband s of channel c inside the tile's bytes: s = 0   */
/*    the low-pass band of level 3 (w_3 h_3 fields of `precision` bits, MSB  */
/*    first, row-major, each stored as int16_t: values above 32767 wrap;     */
/*    `bytes` = 8 ceil(w_3 h_3 precision / 64), :657-666), s = 1-3 / 4-6 /   */
/*    7-9 the high-pass bands 1..3 of level 3 / 2 / 1 (`bytes` = the whole   */
/*    chunk, :798-799; `quant` the band's Quantization).                     */
/*    A high-pass band is a sequence of symbols: a word of the code book,    */
/*    then one sign bit when the word's value is not 0 (1 = negative); it    */
/*    stands for `count` coefficients value * quant, row-major.  The band    */
/*    must give exactly w_k h_k coefficients, followed by the end marker     */
/*    (value +1, count 0).  A band's status, the first that applies in       */
/*    stream order (the bit reader refills four bytes at a time, bytes       */
/*    behind the chunk read as zeros; BitStreamer.h:100-132):                */
/*      RSX_ERR_INPUT_OVERFLOW   a symbol that starts more than              */
/*                               32 floor((bytes + 8) / 4) bits into the     */
/*                               chunk ("Buffer overflow read")              */
/*      RSX_ERR_BAD_HUFFMAN_CODE 26 bits that begin no word of the book      */
/*      RSX_ERR_VALUE_RANGE      value * quant outside int16_t (:714-718;    */
/*                               the end marker itself is not multiplied)    */
/*      RSX_ERR_INVALID_ARG      a count of 0 in front of the last           */
/*                               coefficient, a run that reaches past it,    */
/*                               anything but the end marker behind it       */
/*    Each level turns its four bands into band 0 of the level below (the    */
/*    last one into the channel plane): reconstructPass down the columns     */
/*    (:183-232; band 2 over band 0, band 3 over band 1, results truncated   */
/*    to int16_t), combineLowHighPass along the rows (:234-287) with         */
/*    descaleShift = 2 where prescale[c][k - 1] == 2, else 0 (:364); level 1 */
/*    clamps to 0..16383.  Band 0 of levels 2 and 1 is the 2 w_(k+1) x       */
/*    2 h_(k+1) result of the level above, read as w_k x h_k.  The merge     */
/*    (:875-931): per 2x2 cell gs = plane 0, rg / bg / gd = planes 1..3      */
/*    minus 2048; r = gs + 2 rg, b = gs + 2 bg, g1 = gs + gd, g2 = gs - gd,  */
/*    each through log_table[clamp(v, 0, 4095)]; RGGB stores r g1 / g2 b,    */
/*    GBRG g1 b / r g2.  When any band fails NOTHING is written (the         */
/*    reference throws before combineFinalLowpassBands); the job's status is */
/*    that of its first failing band in (channel, subband) order.  Pitch     */
/*    padding and everything outside the image are never written.            */
/*    The code book: the caller's words with `value` already decompanded     */
/*    (initPrefixCodeDecoder, :437-462); the library holds none.  Refused    */
/*    (RSX_ERR_INVALID_ARG): more than 264 words or none, a size outside     */
/*    1..26, bits that do not fit the size, a count above 511, |value| above */
/*    1023 (the 10 bits a 19-bit code value leaves above the count; the      */
/*    reference's book reaches 1023), words that are not prefix-free.        */
/*    rsx_vc5_validate, in this order: desc, log_table or codes NULL; cpp    */
/*    != 1; dim_x or dim_y <= 0, odd, or above 65534; pitch_bytes < 2 dim_x; */
/*    phase not 0 / 1; a refused code book -> RSX_ERR_INVALID_ARG; dim_x or  */
/*    dim_y < 34 -> RSX_ERR_UNSUPPORTED (a level narrower or shorter than 3: */
/*    the reference's edge filters then read outside its arrays; the CPU     */
/*    gets the tile); then per channel and subband: a low-pass precision     */
/*    outside 8..16 -> RSX_ERR_INVALID_ARG; a band that does not lie inside  */
/*    in_bytes, a low-pass band of fewer than 8 ceil(w_3 h_3 precision / 64) */
/*    bytes, a high-pass chunk of fewer than 4 bytes (the bit reader's       */
/*    minimum) -> RSX_ERR_IO.                                                */
/*    The code book and the log table are copied during the call (or at plan */
/*    creation).                                                             */
/* ------------------------------------------------------------------------ */
typedef struct rsx_vc5_code {
  uint32_t bits;  /* the word, right-justified */
  uint8_t size;   /* its length in bits */
  uint16_t count; /* run length; 0: the end marker */
  int16_t value;  /* decompanded */
} rsx_vc5_code;

typedef struct rsx_vc5_band {
  uint64_t offset; /* of the chunk inside the tile's bytes */
  uint32_t bytes;
  int16_t quant;      /* high-pass bands */
  uint16_t precision; /* the low-pass band */
} rsx_vc5_band;

typedef struct rsx_vc5_desc {
  int32_t phase;             /* 0 RGGB, 1 GBRG */
  const uint16_t* log_table; /* mVC5LogTable (:464-488), 4096 entries, white level included */
  const rsx_vc5_code* codes;
  int32_t n_codes;
  rsx_vc5_band bands[4][10]; /* [channel][subband number] */
  uint8_t prescale[4][3];    /* [channel][level - 1], as parseVC5 left them (:567-576) */
} rsx_vc5_desc;

int rsx_vc5_validate(const rsx_vc5_desc* desc, const rsx_image* img, size_t in_bytes);
int rsx_vc5_decompress(rsx_ctx* ctx, const rsx_vc5_desc* desc, const uint8_t* in, size_t in_bytes,
                       const rsx_image* img);

/* ------------------------------------------------------------------------ */
/* 4e. AbstractDngDecompressor, compression 0x884c: lossy (baseline) JPEG    */
/*    (placed here, next to the other tile codecs; 4d was taken)             */
/*    replaces JpegDecompressor::decode(offX, offY) (decompressThread        */
/*    <0x884c> -> decompressors/JpegDecompressor.cpp:128-170): libjpeg's     */
/*    jpeg_read_header and jpeg_start_decompress with every default left     */
/*    alone (JDCT_ISLOW, fancy upsampling, RGB out for three components,     */
/*    grey for one), all scanlines, then the first min(dim_x - off_x, width) */
/*    pixels of the first min(dim_y - off_y, height) rows widened to 16 bits */
/*    at (off_y, cpp * off_x).  Nothing else of the image is written, its    */
/*    pitch padding included.  "libjpeg" is libjpeg-turbo's default decoder, */
/*    bit for bit; IJG libjpeg 9 upsamples differently.                      */
/*    rsx_dng_jpeg_validate, in this order: no tile, no bytes, an image that */
/*    cannot hold 16-bit samples (no pixels, cpp < 1, an odd pitch_bytes,    */
/*    pitch_bytes < 2 cpp dim_x), off_x >= dim_x or off_y >= dim_y           */
/*    -> RSX_ERR_INVALID_ARG; a tile of 4 GiB or more -> RSX_ERR_UNSUPPORTED;*/
/*    then the markers up to SOS in stream order:                            */
/*      RSX_ERR_IO           no SOI; a marker that is not there; a segment   */
/*                           past the end; a DQT or DHT index above 3, a Pq  */
/*                           above 1, a short table; a second SOF; a         */
/*                           precision other than 8 or 12; zero dimensions   */
/*                           or components; a sampling factor outside 1..4;  */
/*                           an SOS without SOF, with an unknown component,  */
/*                           or naming a table that is not there; EOI or     */
/*                           RSTn in the header                              */
/*      RSX_ERR_UNSUPPORTED  SOF2 and above (progressive, lossless,          */
/*                           arithmetic); 12 bits; two or four components; a */
/*                           scan that does not hold all components in frame */
/*                           order (several scans); Ss, Se, Ah, Al other     */
/*                           than 0, 63, 0, 0; sampling other than luma      */
/*                           h, v in {1, 2} (not 1 x 2) with both chroma     */
/*                           1 x 1, or all 1 x 1 for RGB                     */
/*    then components != cpp -> RSX_ERR_INVALID_ARG (the reference's         */
/*    ThrowRDE), and Huffman counts that are no prefix code or a DC symbol   */
/*    above 15 -> RSX_ERR_IO.                                                */
/*    The colour space is default_decompress_parms': one component is grey;  */
/*    of three, JFIF seen -> YCbCr; else Adobe seen -> transform 0 RGB,      */
/*    otherwise YCbCr; else ids 'R','G','B' -> RGB, anything else YCbCr.     */
/*    Per-tile status of a run, the largest over the tile's segments (a      */
/*    segment is the scan, or one restart interval).  Where libjpeg warns    */
/*    and goes on, the tile is refused:                                      */
/*      RSX_ERR_BAD_HUFFMAN_CODE  a code that is not in the table; a         */
/*                                coefficient index past 63                  */
/*      RSX_ERR_RESTART_MARKER    a marker in the data that is not the RSTn  */
/*                                expected (modulo 8) at a restart interval  */
/*      RSX_ERR_INPUT_OVERFLOW    data that ends before the last MCU, or     */
/*                                inside a segment; no EOI                   */
/*      RSX_ERR_UNSUPPORTED       a DC value outside 16 bits, a dequantised  */
/*                                coefficient or a value behind the column   */
/*                                pass outside +-16383 (what no encoder      */
/*                                makes from 8-bit pixels, and where         */
/*                                libjpeg-turbo's SIMD and C code differ)    */
/*    Bytes behind EOI, and bytes of a segment behind its last MCU, are      */
/*    ignored.  A tile that is not RSX_OK writes NOTHING into the image; the */
/*    others are written.  The call returns RSX_ERR_TILE_ERRORS if any tile  */
/*    failed.  One upload of the packed tile bytes, one launch sequence, one */
/*    download; one host call in rsx_ctx_host_calls.                         */
/* ------------------------------------------------------------------------ */
typedef struct rsx_dng_jpeg_tile {
  const uint8_t* in; /* the tile's JPEG stream, SOI first */
  size_t in_bytes;
  uint32_t off_x, off_y; /* e.offX, e.offY: pixels */
} rsx_dng_jpeg_tile;

#define RSX_JPEG_GREY 0
#define RSX_JPEG_YCBCR 1
#define RSX_JPEG_RGB 2

typedef struct rsx_dng_jpeg_info {
  uint32_t width, height;    /* the frame's */
  int32_t components;        /* 1 or 3 = output_components */
  int32_t h_samp, v_samp;    /* of the first component against the others */
  int32_t colour_space;      /* RSX_JPEG_*: what the stream holds */
  uint32_t restart_interval; /* MCUs, 0: none */
  uint32_t n_segments;       /* entropy segments = wavefronts of the block kernel */
} rsx_dng_jpeg_info;

/* `info` may be NULL; it is filled when the status is RSX_OK */
int rsx_dng_jpeg_validate(const rsx_dng_jpeg_tile* tile, const rsx_image* img,
                          rsx_dng_jpeg_info* info);
int rsx_dng_decompress_jpeg(rsx_ctx* ctx, int n_tiles, const rsx_dng_jpeg_tile* tiles,
                            const rsx_image* img, int32_t* tile_status);

/* ------------------------------------------------------------------------ */
/* 4d. DngDecoder behind the tiles: OpcodeList1 and the LinearizationTable   */
/*    replaces, in DngDecoder::handleMetadata (decoders/DngDecoder.cpp       */
/*    :591-615), DngOpcodes::applyOpCodes (common/DngOpcodes.cpp) and        */
/*    RawImageData::sixteenBitLookup() -> RawImageDataU16::doLookup          */
/*    (common/RawImageDataU16.cpp:488-519).  Every opcode the reference      */
/*    implements reads and writes only the sample it stands on, so the list  */
/*    and the look-up are ONE pass on the device.                            */
/*    The caller hands over the OpcodeList1 entry's bytes as they are in the */
/*    file (big-endian; NULL / 0 bytes: none, as for an entry of count 0),   */
/*    the LinearizationTable's values (1..65536; NULL / 0: none -- also what */
/*    a caller with uncorrectedRawValues passes), the UNCROPPED image (uint16 */
/*    or, is_f32, binary32) and the image's crop in pixels as it stands      */
/*    behind handleMetadata's ActiveArea and DefaultCrop subFrames.          */
/*    The list is parsed here, with the reference's checks in its order.     */
/*    What a check throws decides the outcome: DngDecoder catches only       */
/*    RawDecoderException around the list (:593-604), logs it and goes on to */
/*    the look-up; an IOException of the ByteStream fails the file.          */
/*    IOException -> the call returns RSX_ERR_IO, nothing is applied, the    */
/*    image is untouched: the list shorter than its count field; in the      */
/*    first walk over the list an opcode header or an opcode's size that     */
/*    leaves the list (skipBytes); any getU32 / getU16 / get<float> /        */
/*    get<double> of an opcode that leaves the opcode's own bytes (getStream */
/*    gave it exactly `size`); FixBadPixelsList's skipBytes(points, 8) and   */
/*    skipBytes(rects, 16); MapPolynomial's check(8 (degree + 1));           */
/*    Delta / Scale's check(count, 4).                                       */
/*    RawDecoderException while the list is CONSTRUCTED -> RSX_OK, the       */
/*    result's list_status = RSX_ERR_INVALID_ARG with a reason, n_applied =  */
/*    0: a rectangle not inside the crop the opcode meets, or bottom < top,  */
/*    right < left (REASON_ROI; TrimBounds, every pixel opcode, the          */
/*    rectangles of FixBadPixelsList against the uncropped image); planes == */
/*    0 or firstPlane + planes > cpp (REASON_PLANES); a pitch of 0 or above  */
/*    the ROI's extent (REASON_PITCH); MapTable with 0 or more than 65536    */
/*    entries (REASON_TABLE_SIZE); MapPolynomial of degree above 8           */
/*    (REASON_POLY_DEGREE); a delta count other than ceil(extent / pitch)    */
/*    (REASON_DELTA_COUNT); a non-finite delta (REASON_DELTA_NOT_FINITE); a  */
/*    point of FixBadPixelsList outside the uncropped image                  */
/*    (REASON_BAD_POINT); a code of 0 or above 13 (REASON_UNKNOWN_OPCODE);   */
/*    WarpRectilinear, WarpFisheye, FixVignetteRadial or GainMap (1, 2, 3,   */
/*    9) without flag bit 0 (REASON_UNSUPPORTED_OPCODE); bytes of an opcode  */
/*    left unread (REASON_INCONSISTENT_LENGTH -- which is also what an       */
/*    OPTIONAL opcode 1, 2, 3 or 9 gets unless it is empty: the reference    */
/*    skips its constructor, not its bytes).                                 */
/*    RawDecoderException from an opcode's setup() or apply() -> RSX_OK,     */
/*    list_status = RSX_ERR_INVALID_ARG, n_applied = the number of list      */
/*    entries in front of it, and those STAY applied: MapTable,              */
/*    MapPolynomial or FixBadPixelsConstant on an F32 image                  */
/*    (REASON_SETUP_NOT_U16); FixBadPixelsConstant with cpp > 1              */
/*    (REASON_SETUP_CPP); on a uint16 image an offset with |f| > 1.0 or a    */
/*    scale outside 0 .. (2^31 - 513) / 65535 / 1024 (REASON_SETUP_DELTA_    */
/*    RANGE); a TrimBounds of no area (REASON_TRIM_EMPTY: subFrame's "No     */
/*    positive crop area").                                                  */
/*    Either way the look-up follows.                                        */
/*    The opcodes.  ROI (top, left, bottom, right), firstPlane, planes,      */
/*    rowPitch, colPitch; PixelOpcode::applyOP (:391-407) touches row crop.y */
/*    + top + rowPitch y, sample firstPlane + (left + colPitch x) cpp + p of */
/*    the cropped row, y < ceil(height / rowPitch), x < ceil(width /         */
/*    colPitch), p < planes; the delta index is x or y.  MapTable (7): the   */
/*    table, filled up with its last entry.  MapPolynomial (8): a table of   */
/*    uint16(clamp(sum_j c_j pow(i / 65536.0, j) 65535.5, 0, 65535)) in      */
/*    binary64 (a NaN gives 0 here; the reference's conversion is            */
/*    undefined).  DeltaPerRow / Column (10, 11): uint16 clampBits(int(      */
/*    65535.0F f) + v, 16); F32 f + v.  ScalePerRow / Column (12, 13):       */
/*    uint16 clampBits((int(1024.0F f) v + 512) >> 10, 16); F32 f v.         */
/*    FixBadPixelsConstant (4) changes no pixel: every pixel of the crop it  */
/*    meets whose value equals the constant is listed as (crop.x | crop.y << */
/*    16) + (row << 16 | col), row-major.  TrimBounds (6) moves the crop for */
/*    every later opcode; the result carries the crop behind the applied     */
/*    part of the list, for the caller's subFrame.  FixBadPixelsList (5):    */
/*    y << 16 | x of its points and of every pixel of its rectangles, in     */
/*    uncropped coordinates.                                                 */
/*    The bad-pixel positions: what mRaw->mBadPixelPositions gains, in the   */
/*    reference's final order -- FixBadPixelsConstant appends, FixBadPixels- */
/*    List inserts its entries at the FRONT, in file order.  result->n_bad   */
/*    is always the exact count; when it exceeds bad_cap the image is still  */
/*    complete and correct, the call reports RSX_ERR_UNSUPPORTED and the     */
/*    list's contents are unspecified (rsx_panasonic_v4_decompress's         */
/*    contract).  `bad` NULL with bad_cap 0 is allowed.                      */
/*    The look-up.  The table is TableLookUp::setTable with dither (common/  */
/*    TableLookUp.cpp:68-84): base = clampBits(center - (upper - lower + 2)  */
/*    / 4, 16), delta = upper - lower with lower / upper clamped against the */
/*    centre; behind the table its last value, delta 0.  doLookup differs    */
/*    from the store-time look-up of sections 3i and 3m: per row v = (dim_x  */
/*    + 13 y) ^ 0x45694584, per sample FIRST v = 15700 (v & 65535) + (v >>   */
/*    16), then pixel = clampBits(base + ((delta (v & 2047) + 1024) >> 12),  */
/*    16).  It covers EVERY row of the UNCROPPED image at the full uncropped */
/*    width x cpp, whatever the crop: sixteenBitLookup passes cropped = true */
/*    to startWorker, but APPLY_LOOKUP carries RawImageWorkerTask::          */
/*    FULL_IMAGE (common/RawImage.h:61, RawImage.cpp:270-279), and doLookup  */
/*    indexes the uncropped array.  Neither ActiveArea nor a TrimBounds      */
/*    keeps a row or a column out of it.                                     */
/*    rsx_dng_post_validate, in this order: desc or img NULL; cpp outside    */
/*    1..4, dim_x or dim_y <= 0; pitch_bytes < dim_x cpp (2 or 4) or not a   */
/*    multiple of the sample size; a crop of no area or outside the image;   */
/*    opcodes NULL with opcodes_bytes != 0, table NULL with table_count !=   */
/*    0, table_count > 65536 -> RSX_ERR_INVALID_ARG; a table on an F32 image */
/*    (the reference logs "not implemented" from a worker), dim_x cpp or     */
/*    dim_y >= 2^24, dim_x + 13 dim_y >= 2^20 -> RSX_ERR_UNSUPPORTED; then   */
/*    the list: RSX_ERR_IO as above; more than 2^26 FixBadPixelsList         */
/*    positions, more than 16 tables, more than RSX_DNG_POST_MAX_PIXEL_OPS   */
/*    pixel opcodes (4, 7, 8, 10..13) in the applied part ->                 */
/*    RSX_ERR_UNSUPPORTED (the caller keeps the host path).  It fills the    */
/*    result and hands out the positions that need no pixel (FixBadPixels-   */
/*    List); no device.                                                      */
/*    On any status but RSX_OK (and RSX_ERR_UNSUPPORTED for bad_cap) the     */
/*    image is untouched.  Pitch padding is never written.                   */
/*    rsx_dng_post works in place; img->data may be a host pointer (the rows */
/*    go up, are processed and come back) or a device pointer (the call      */
/*    returns when the pass is done).  Through host pointers the pass costs  */
/*    a round trip over the link; deflate and VC-5 images, whose host calls  */
/*    download their tiles, use it on a device pointer or as a plan behind   */
/*    their own plans.                                                       */
/* ------------------------------------------------------------------------ */
#define RSX_DNG_POST_MAX_PIXEL_OPS 16
typedef enum rsx_dng_post_reason {
  RSX_DNG_POST_REASON_NONE = 0,
  RSX_DNG_POST_REASON_ROI = 1,
  RSX_DNG_POST_REASON_PLANES = 2,
  RSX_DNG_POST_REASON_PITCH = 3,
  RSX_DNG_POST_REASON_DELTA_COUNT = 4,
  RSX_DNG_POST_REASON_DELTA_NOT_FINITE = 5,
  RSX_DNG_POST_REASON_TABLE_SIZE = 6,
  RSX_DNG_POST_REASON_POLY_DEGREE = 7,
  RSX_DNG_POST_REASON_UNKNOWN_OPCODE = 8,
  RSX_DNG_POST_REASON_UNSUPPORTED_OPCODE = 9,
  RSX_DNG_POST_REASON_INCONSISTENT_LENGTH = 10,
  RSX_DNG_POST_REASON_BAD_POINT = 11,
  RSX_DNG_POST_REASON_SETUP_NOT_U16 = 12,
  RSX_DNG_POST_REASON_SETUP_CPP = 13,
  RSX_DNG_POST_REASON_SETUP_DELTA_RANGE = 14,
  RSX_DNG_POST_REASON_TRIM_EMPTY = 15
} rsx_dng_post_reason;

typedef struct rsx_dng_post_desc {
  const uint8_t* opcodes; /* the OpcodeList1 entry's bytes */
  uint32_t opcodes_bytes;
  uint32_t table_count;   /* LinearizationTable entries */
  const uint16_t* table;
  int32_t is_f32;         /* RawImageType::F32 */
  int32_t crop_x, crop_y, crop_w, crop_h; /* mOffset and dim, pixels */
  int32_t reserved;
} rsx_dng_post_desc;

typedef struct rsx_dng_post_result {
  int32_t list_status; /* RSX_OK, or RSX_ERR_INVALID_ARG: the reference logs it and goes on */
  int32_t list_reason; /* rsx_dng_post_reason */
  int32_t n_opcodes;   /* entries of a list that constructed */
  int32_t n_applied;   /* entries applied */
  int32_t crop_x, crop_y, crop_w, crop_h; /* behind the applied TrimBounds */
  uint64_t n_bad;
} rsx_dng_post_result;

int rsx_dng_post_validate(const rsx_dng_post_desc* desc, const rsx_image* img,
                          rsx_dng_post_result* result, uint32_t* bad, uint32_t bad_cap);
int rsx_dng_post(rsx_ctx* ctx, const rsx_dng_post_desc* desc, const rsx_image* img,
                 rsx_dng_post_result* result, uint32_t* bad, uint32_t bad_cap);
/* The tile fan-outs of section 4 with the pass on the decoded image on the device and ONE
 * download -- the form the pass is for.  The tiles, any number of them, must tile the image: each
 * inside it, no two sharing a sample, all of it covered (RSX_ERR_UNSUPPORTED otherwise, before
 * anything is uploaded or decoded).  tile_status (and tile_consumed) are written only by a call
 * that wrote the image -- RSX_OK, RSX_ERR_TILE_ERRORS, or RSX_ERR_UNSUPPORTED for a position
 * list past bad_cap; with any other status nothing was downloaded and they are as the caller
 * set them, so a caller falls back to the plain call on anything but RSX_OK and
 * RSX_ERR_TILE_ERRORS.  If any tile fails the call behaves exactly like the plain call:
 * the good tiles are written, it returns the plain call's status, NOTHING of the list or the
 * look-up is applied and the result carries the parse alone; the caller's CPU path, list
 * included, takes over as it does for the plain call.  A list that fails the file (RSX_ERR_IO)
 * or that this core refuses is returned before anything is decoded.  The uncompressed form also
 * refuses (RSX_ERR_UNSUPPORTED, nothing written) packed tiles with crop_x != 0: the reference's
 * packed paths write them from column 0, on top of their neighbours, and only the plain call
 * keeps the order in which they land. */
int rsx_dng_decompress_ljpeg_post(rsx_ctx* ctx, int n_tiles, const rsx_dng_ljpeg_tile* tiles,
                                  const rsx_dng_post_desc* desc, const rsx_image* img,
                                  int32_t* tile_status, uint32_t* tile_consumed,
                                  rsx_dng_post_result* result, uint32_t* bad, uint32_t bad_cap);
int rsx_dng_decompress_uncompressed_post(rsx_ctx* ctx, int n_tiles,
                                         const rsx_dng_unpack_tile* tiles,
                                         const rsx_dng_post_desc* desc, const rsx_image* img,
                                         int32_t* tile_status, rsx_dng_post_result* result,
                                         uint32_t* bad, uint32_t bad_cap);

/* ------------------------------------------------------------------------ */
/* 5. RawImageData::fixBadPixels: the last step of RawDecoder::decodeRaw     */
/*    (decoders/RawDecoder.cpp:327-328; common/RawImage.cpp:201-239,         */
/*    :297-323, common/RawImageDataU16.cpp:399-485,                          */
/*    common/RawImageDataFloat.cpp:177-260).                                 */
/*                                                                           */
/*    A position is y << 16 | x in UNCROPPED coordinates (mBadPixelPositions)*/
/*    and the map is mBadPixelMap: rows of map_pitch = roundUp(ceil(dim_x /  */
/*    8), 16) bytes, bit x & 7 of byte x >> 3 (createBadPixelMap).  The      */
/*    stage ORs the positions into the map (duplicates are harmless, the map */
/*    may already hold bits: map_in), then gives every marked pixel with     */
/*    x < 32 ((dim_x + 15) / 32) -- fixBadPixelsThread scans that many       */
/*    blocks of 32, so the marked pixels of a last partial block of 1..16    */
/*    columns stay as they are, and stay marked -- the value of              */
/*    fixBadPixel: from the nearest unmarked pixel to the left, to the       */
/*    right, above and below, stepping by 2 when img->is_cfa, by 1           */
/*    otherwise, weighted by distance.  uint16: truncating integer weights   */
/*    of 256ths, a shift of 7 plus one per axis with a neighbour, clamped to */
/*    16 bits; a pixel without any neighbour becomes 0.  F32 (is_f32): the   */
/*    walk passes unmarked pixels with a negative value (their distance      */
/*    counts, their value does not; -0.0 and NaN stop it), every binary32    */
/*    operation is rounded on its own, and a NaN result is stored as         */
/*    0xFFC00000, what the reference's invalid operation gives on x86-64.    */
/*    The stage reads only unmarked pixels and writes only marked ones, so   */
/*    its result does not depend on the order of the pixels.  It always      */
/*    works on the uncropped image, after everything else: for DNG behind    */
/*    the opcode list and the look-up of section 4d.  Bit-exact against the  */
/*    reference (tests/golden/bad_pixels_ref.json).                          */
/*                                                                           */
/*    cpp > 1 is RSX_ERR_UNSUPPORTED and the caller keeps the host path: the */
/*    reference indexes img(y, x + component) with the PIXEL's x, not x cpp, */
/*    so its writes land on samples other fixes read, and its row-split      */
/*    threads race on them -- there is no result to be bit-exact with.       */
/*                                                                           */
/*    rsx_bad_pixels_validate, in this order: desc or img NULL (or positions */
/*    NULL with n_positions != 0); cpp < 1, dim_x or dim_y <= 0, pitch_bytes */
/*    below dim_x cpp samples or no multiple of the sample size (2, or 4 for */
/*    is_f32) -> RSX_ERR_INVALID_ARG; cpp > 1 -> RSX_ERR_UNSUPPORTED; dim_x  */
/*    or dim_y > 65536 -> RSX_ERR_UNSUPPORTED; map_pitch other than          */
/*    createBadPixelMap's (0 is allowed when neither map_in nor map_out is   */
/*    given) -> RSX_ERR_INVALID_ARG; a position, or a bit of map_in, at x >= */
/*    dim_x or y >= dim_y -> RSX_ERR_INVALID_ARG (the reference only asserts */
/*    and would write outside its map).  On any status but RSX_OK the image  */
/*    and map_out are untouched.                                             */
/*    With no positions and no map_in the reference makes no map and touches */
/*    nothing: RSX_OK, n_bad = n_fixed = 0, map_made = 0, map_out untouched. */
/*    Otherwise map_made = 1 and map_out (if given) receives the map as      */
/*    mBadPixelMap holds it afterwards: map_pitch dim_y bytes.               */
/*    rsx_bad_pixels_fix works in place; img->data may be a host pointer     */
/*    (the rows go up and come back) or a device pointer (the call returns   */
/*    when the pass is done); positions, map_in and map_out are host memory. */
/* ------------------------------------------------------------------------ */
typedef struct rsx_bad_pixels_desc {
  const uint32_t* positions; /* may be NULL with n_positions 0 */
  uint32_t n_positions;
  uint32_t map_pitch;
  const uint8_t* map_in; /* may be NULL */
  uint8_t* map_out;      /* may be NULL */
  int32_t is_f32;
  int32_t reserved;
} rsx_bad_pixels_desc;

typedef struct rsx_bad_pixels_result {
  uint64_t n_bad;   /* distinct marked pixels */
  uint64_t n_fixed; /* ... of which were given a value */
  int32_t map_made; /* 0: the reference would have made no map */
  int32_t reserved;
} rsx_bad_pixels_result;

int rsx_bad_pixels_validate(const rsx_bad_pixels_desc* desc, const rsx_image* img);
int rsx_bad_pixels_fix(rsx_ctx* ctx, const rsx_bad_pixels_desc* desc, const rsx_image* img,
                       rsx_bad_pixels_result* result);
/* rsx_panasonic_v4_decompress (section 3l), then the stage on the decoded image on the device,
 * ONE download.  With desc->zero_is_bad the bad pixels are exactly the zero pixels of the decoded
 * image, so the map is marked from the image and the call depends on no list capacity; without
 * the flag, or with no zero pixel in the image, the reference makes no map (map_made = 0, map_out
 * untouched).  map_out (may be NULL; map_pitch as above,
 * 0 allowed without map_out) receives the map for the caller's mBadPixelMap, result (may be NULL)
 * the counts.  Statuses as rsx_panasonic_v4_decompress, plus the stage's image checks (an odd
 * pitch_bytes, a dimension past 65536); on anything but RSX_OK nothing is written. */
int rsx_panasonic_v4_decompress_fixed(rsx_ctx* ctx, const rsx_panasonic_v4_desc* desc,
                                      const uint8_t* in, size_t in_bytes, const rsx_image* img,
                                      uint8_t* map_out, uint32_t map_pitch,
                                      rsx_bad_pixels_result* result);

/* rsx_dng_post, rsx_dng_decompress_ljpeg_post and rsx_dng_decompress_uncompressed_post (section
 * 4d) with the bad-pixel stage behind the look-up, on the positions the pass composed, in front
 * of the one download: the same arguments plus map_out (may be NULL; createBadPixelMap's pitch
 * times dim_y bytes, written only when the positions are not empty -- the reference makes no map
 * otherwise).  Each obeys every status rule of the call it extends: a failing tile, a list that
 * fails the file or a refused list apply nothing, fix included.  A position list past bad_cap
 * leaves the image as the _post call leaves it, UNFIXED, with RSX_ERR_UNSUPPORTED: the caller runs
 * fixBadPixels itself.  An image with cpp > 1 whose list yields positions (FixBadPixelsList
 * entries; FixBadPixelsConstant refuses such images itself) returns RSX_ERR_UNSUPPORTED before
 * anything is decoded or written, and the caller uses the _post call and the host pass. */
int rsx_dng_finish(rsx_ctx* ctx, const rsx_dng_post_desc* desc, const rsx_image* img,
                   rsx_dng_post_result* result, uint32_t* bad, uint32_t bad_cap, uint8_t* map_out);
int rsx_dng_decompress_ljpeg_finish(rsx_ctx* ctx, int n_tiles, const rsx_dng_ljpeg_tile* tiles,
                                    const rsx_dng_post_desc* desc, const rsx_image* img,
                                    int32_t* tile_status, uint32_t* tile_consumed,
                                    rsx_dng_post_result* result, uint32_t* bad, uint32_t bad_cap,
                                    uint8_t* map_out);
int rsx_dng_decompress_uncompressed_finish(rsx_ctx* ctx, int n_tiles,
                                           const rsx_dng_unpack_tile* tiles,
                                           const rsx_dng_post_desc* desc, const rsx_image* img,
                                           int32_t* tile_status, rsx_dng_post_result* result,
                                           uint32_t* bad, uint32_t bad_cap, uint8_t* map_out);

/* ------------------------------------------------------------------------ */
/* 6. RawImageData::scaleBlackWhite: the third call of the documented flow   */
/*    (common/RawImageDataU16.cpp:60-392, common/RawImageDataFloat.cpp:      */
/*    51-170, common/RawImage.cpp:270-295, :339-371).                        */
/*                                                                           */
/*    img describes the UNCROPPED image; the descriptor carries what         */
/*    RawImageData holds when the call is made, the result what the          */
/*    reference leaves in its members.  Everything is as the code is         */
/*    written, quirks included, and bit-exact against the reference          */
/*    (tests/golden/scale_ref.json).  The row split of startWorker does not  */
/*    enter the result: every row seeds its own generator.                   */
/*                                                                           */
/*    uint16, in this order:                                                 */
/*    (1) the estimate, when (no areas, no separate levels and black_level   */
/*    < 0) or has_white == 0: min and max over cropped rows 250 .. crop_y -  */
/*    250 and cropped samples 250 + col, col in 250 .. (crop_x - 250) cpp    */
/*    (the reference's double offset); an empty window gives 65536 and 0.    */
/*    (2) the skip rule: (no areas, black_level 0, white 65535, no separate  */
/*    levels) or an empty crop -> skipped = 1, the image untouched.          */
/*    (3) calculateBlackAreas when no separate levels are given: sizes       */
/*    rounded down to even; a horizontal area counts the single sample       */
/*    img(y, off_x) once per cropped column into the histogram of the row    */
/*    and column parity; a vertical area counts img(y, area.offset) once per */
/*    column of the area; the cells are 16 bits and wrap; totalpixels / 8    */
/*    and the median walk; not CFA: the rounded average; no counted pixel:   */
/*    all four become black_level.                                           */
/*    (4) the pass.  host_sse2 (WITH_SSE2 && Cpuid::SSE2() of the caller's   */
/*    build) and app_scale = 65535.0F / (white - black_separate[0]) < 63:    */
/*    the SSE2 variant (variant 1), over cropped rows and UNCROPPED samples  */
/*    0 .. roundDown(dim_x, 8) of a row (for cpp > 1 only these first dim_x  */
/*    samples): saturating subtraction, 10-bit multipliers packed two to a   */
/*    word as written, black level bls(off_x & 1) for uncropped-even         */
/*    columns, eight 16-bit generators a row stepped once per block of       */
/*    eight.  Otherwise the plain variant (variant 0), over cropped samples  */
/*    0 .. crop_x cpp, with the generator v = 18000 (v & 65535) + (v >> 16)  */
/*    seeded crop_x + y 36969 per row.  Where its int arithmetic leaves      */
/*    int32 (undefined in the reference) it wraps, and n_wrapped counts      */
/*    those samples.  dither == 0: no generator in either.                   */
/*                                                                           */
/*    F32 (is_f32, variant 2): the estimate (no areas, no separate levels,   */
/*    black_level < 0) is the minimum over cropped rows 150 cpp .. crop_y -  */
/*    150, cropped samples 150 .. (crop_x - 150) cpp, converted with         */
/*    static_cast<int>; no skip rule; the pass is (p - sub) * mul over the   */
/*    cropped samples, two roundings.                                        */
/*                                                                           */
/*    rsx_scale_validate, in this order: desc or img NULL (or areas NULL     */
/*    with n_areas != 0); cpp < 1, dim_x or dim_y <= 0, pitch_bytes below    */
/*    dim_x cpp samples or no multiple of the sample size; a crop outside    */
/*    the image -> RSX_ERR_INVALID_ARG; dim_x or dim_y > 65536 (or cpp > 4)  */
/*    -> RSX_ERR_UNSUPPORTED; F32 with has_white == 0 (the reference            */
/*    dereferences it) or with areas (its answer is a sequential binary32    */
/*    sum) -> RSX_ERR_UNSUPPORTED; uint16, when the areas would be used: an  */
/*    area past the image (the reference's ThrowRDE) -> RSX_ERR_INVALID_ARG. */
/*    Then, from the image, after the estimate and the areas and before      */
/*    anything is written: F32 with a NaN inside the estimate window         */
/*    (std::min's result would depend on the scan order) or a minimum below  */
/*    int -> RSX_ERR_UNSUPPORTED; white - black_separate[i] <= 0 for any i   */
/*    (the reference's division by zero or negative scale) ->                */
/*    RSX_ERR_UNSUPPORTED; plain variant with a row seed crop_x + y 36969    */
/*    past INT32_MAX -> RSX_ERR_UNSUPPORTED.  On any status but RSX_OK the   */
/*    image is untouched, the result zero, and the caller keeps the host     */
/*    path.                                                                  */
/*    rsx_scale_black_white works in place; img->data may be a host pointer  */
/*    (the rows go up and come back) or a device pointer (the call returns   */
/*    when the pass is done).  Every step runs on the device without a host  */
/*    round trip in between; areas is host memory.                           */
/* ------------------------------------------------------------------------ */
typedef struct rsx_scale_area {
  uint32_t offset;
  uint32_t size;
  int32_t is_vertical;
  int32_t reserved;
} rsx_scale_area;

typedef struct rsx_scale_desc {
  int32_t off_x, off_y;   /* mOffset */
  int32_t crop_x, crop_y; /* dim */
  int32_t is_f32;
  int32_t black_level; /* -1: unset */
  int32_t has_white;
  int32_t white_point;
  int32_t has_separate;
  int32_t black_separate[4];
  uint32_t n_areas;
  const rsx_scale_area* areas; /* may be NULL with n_areas 0 */
  int32_t dither;              /* mDitherScale */
  int32_t host_sse2;
} rsx_scale_desc;

typedef struct rsx_scale_result {
  int32_t black_level;
  int32_t white_point;
  int32_t black_separate[4];
  int32_t estimated; /* the estimate ran */
  int32_t skipped;   /* "skip, if not needed": the image is untouched */
  int32_t variant;   /* 0 plain, 1 SSE2, 2 F32 */
  int32_t reserved;
  uint64_t n_wrapped;
} rsx_scale_result;

int rsx_scale_validate(const rsx_scale_desc* desc, const rsx_image* img);
int rsx_scale_black_white(rsx_ctx* ctx, const rsx_scale_desc* desc, const rsx_image* img,
                          rsx_scale_result* result);

/* ------------------------------------------------------------------------ */
/* 4f. DngDecoder's branch for lossy DNGs, end to end                        */
/*    (placed here, behind the stages it chains: it needs their types)       */
/*    replaces, for compression 0x884c, the tiles of section 4e, then        */
/*    DngDecoder::handleMetadata (decoders/DngDecoder.cpp:591-634) and       */
/*    RawDecoder::decodeRaw()'s last step (decoders/RawDecoder.cpp:327-328): */
/*    OpcodeList1 (:591-605), the LinearizationTable look-up (:607-615),     */
/*    setBlack (:618, the caller's: it fills `scale`), scaleBlackWhite()     */
/*    (:624), OpcodeList2 (:627-634), fixBadPixels.  Every stage is the      */
/*    stage of section 4d, 6 and 5, bit for bit, on one staged image: ONE    */
/*    upload of the tiles, ONE download.  The caller keeps the metadata tail */
/*    of :635-642 (blackAreas.clear(), black 0, white 65535).                */
/*    Without has_list2 (no OPCODELIST2 entry, or uncorrectedRawValues):     */
/*    what rsx_dng_decompress_ljpeg_post / _finish are for LJPEG tiles, with */
/*    JPEG tiles -- tiles, list 1, look-up, `fix`, the download.  scale,     */
/*    opcodes2 are ignored; result->scale and ->list2 are zero.              */
/*    With has_list2: the scale stage runs behind the look-up on the crop    */
/*    list 1 left: scale.off_x, off_y, crop_x, crop_y must equal list1.crop_x*/
/*    crop_y, crop_w, crop_h (the caller has them from rsx_dng_post_validate */
/*    and needs them for setBlack), scale.is_f32 must be 0 ->                */
/*    RSX_ERR_INVALID_ARG otherwise.  Then list 2, a DngOpcodes list without */
/*    a table whose crop starts where list 1 left it; every rule of section  */
/*    4d for verdicts, reasons and n_applied holds for it.  Unlike list 1,   */
/*    an entry of 0 bytes is not "none": :628 has no `count > 0` guard, the  */
/*    constructor's getU32 throws IOException -> RSX_ERR_IO.                 */
/*    The positions are what mBadPixelPositions holds at the end (common/    */
/*    DngOpcodes.cpp:180 inserts at the front, :320 appends): list 2's       */
/*    FixBadPixelsList entries, list 1's, list 1's constant hits, list 2's   */
/*    constant hits -- the latter taken on the SCALED image.  list1.n_bad +  */
/*    list2.n_bad is always the exact count.                                 */
/*    The checks that need no pixel, in this order (rsx_dng_lossy_validate   */
/*    makes them all, fills both parses and hands out the FixBadPixelsList   */
/*    positions; no device): desc or img NULL, stage1.is_f32 ->              */
/*    RSX_ERR_INVALID_ARG; list 1 as rsx_dng_post_validate; list 2 likewise; */
/*    the scale crop; rsx_scale_validate; fix with cpp > 1 and a FixBad-     */
/*    PixelsList position in either list -> RSX_ERR_UNSUPPORTED (section 5). */
/*    Any of them ends rsx_dng_lossy_decompress before anything is decoded.  */
/*    Then, as the calls the stages extend:                                  */
/*      tiles that parse and do not tile the image (section 4d) ->           */
/*        RSX_ERR_UNSUPPORTED before anything is uploaded;                   */
/*      a tile fails -> the plain call of section 4e: the good tiles are     */
/*        written, RSX_ERR_TILE_ERRORS, stages = 0, the result carries the   */
/*        parses alone;                                                      */
/*      the scale stage refuses from the image's contents (white - black <=  */
/*        0, the row seed) -> the image comes back as stage 1 left it,       */
/*        stages = RSX_DNG_LOSSY_STAGE1, `bad` holds list 1's positions      */
/*        alone and list2.n_bad is 0 (list 2's verdict stays the parse's),   */
/*        RSX_ERR_UNSUPPORTED; the caller goes on from scaleBlackWhite();    */
/*      more positions than bad_cap -> the image complete but UNFIXED,       */
/*        RSX_ERR_UNSUPPORTED, `bad` unspecified (as the _finish calls).     */
/*    RSX_DNG_LOSSY_FIXED is set when `fix` was asked for and the positions  */
/*    fit, also when there were none (the reference then makes no map, and   */
/*    map_out stays untouched).  tile_status is written only by a call that  */
/*    wrote the image.  Pitch padding is never written.  img->data is a host */
/*    pointer.  One host call in rsx_ctx_host_calls.                         */
/* ------------------------------------------------------------------------ */
typedef struct rsx_dng_lossy_desc {
  rsx_dng_post_desc stage1; /* OpcodeList1 + LinearizationTable, as section 4d; is_f32 must be 0 */
  int32_t has_list2;        /* the file has an OPCODELIST2 entry and !uncorrectedRawValues */
  uint32_t opcodes2_bytes;
  const uint8_t* opcodes2;  /* the entry's bytes as in the file */
  rsx_scale_desc scale;     /* what RawImageData holds behind setBlack(); used only with has_list2 */
  int32_t fix;              /* run fixBadPixels behind everything, in front of the download */
  int32_t reserved;
} rsx_dng_lossy_desc;

#define RSX_DNG_LOSSY_STAGE1 1 /* list 1 + look-up applied */
#define RSX_DNG_LOSSY_SCALED 2 /* scaleBlackWhite ran (it may have set result.scale.skipped) */
#define RSX_DNG_LOSSY_LIST2 4
#define RSX_DNG_LOSSY_FIXED 8
typedef struct rsx_dng_lossy_result {
  rsx_dng_post_result list1, list2;
  rsx_scale_result scale;
  rsx_bad_pixels_result fixed;
  uint32_t stages; /* RSX_DNG_LOSSY_*: what the downloaded image has behind it */
  uint32_t reserved;
} rsx_dng_lossy_result;

int rsx_dng_lossy_validate(const rsx_dng_lossy_desc* desc, const rsx_image* img,
                           rsx_dng_lossy_result* result, uint32_t* bad, uint32_t bad_cap);
int rsx_dng_lossy_decompress(rsx_ctx* ctx, int n_tiles, const rsx_dng_jpeg_tile* tiles,
                             const rsx_dng_lossy_desc* desc, const rsx_image* img,
                             int32_t* tile_status, rsx_dng_lossy_result* result, uint32_t* bad,
                             uint32_t bad_cap, uint8_t* map_out);

/* ------------------------------------------------------------------------ */
/* 4g. The image hash of rstest and the sums of rawspeed-identify            */
/*    replaces imgDataHash (utilities/rstest/rstest.cpp:131-146), "md5sum of */
/*    per-line md5sums", and the byte sum and uint16_t sum of                */
/*    utilities/identify/rawspeed-identify.cpp:235-283, on an image that     */
/*    stays on the device: 16 dim_y + 32 bytes come back, not the image.     */
/*    The image is the UNCROPPED one; its samples are sample_bytes = 2       */
/*    (UINT16) or 4 (F32) bytes each (rsx_image has no type field).  With    */
/*    row_bytes = dim_x cpp sample_bytes:                                    */
/*      line[j]    the 16-byte MD5 (RFC 1321) of the row_bytes bytes of row  */
/*                 j as stored (little-endian samples); bytes of the pitch   */
/*                 beyond row_bytes never reach a result;                    */
/*      md5        the MD5 of the 16 dim_y bytes line[0] .. line[dim_y - 1]; */
/*      byte_sum   the sum of all row_bytes dim_y bytes;                     */
/*      sample_sum the sum of all samples read as uint16_t for 2-byte        */
/*                 images, 0 for 4-byte images.                              */
/*    A digest's bytes are the state words A, B, C, D in little-endian order */
/*    (hashlib's digest(); the reference's md5::state_type in memory on a    */
/*    little-endian host).  The reference accumulates both sums in double;   */
/*    both stay below 2^53, so double(sum) is its value exactly.  identify's */
/*    sum of F32 samples is left out: the reference's value depends on how   */
/*    OpenMP splits the rows among threads and combines them, so there is no */
/*    one answer to match.  Results are the same from run to run: nothing is */
/*    added in an order that can vary.                                       */
/*    rsx_image_hash_validate, in this order: img NULL; sample_bytes not 2   */
/*    or 4; cpp < 1, dim_x < 1 or dim_y < 1; pitch_bytes < row_bytes or not  */
/*    a multiple of sample_bytes -> RSX_ERR_INVALID_ARG; row_bytes >= 2^28   */
/*    or dim_y >= 2^24 -> RSX_ERR_UNSUPPORTED (this keeps every MD5 chain    */
/*    far below the upper word of the bit count, which is written as 64 bits */
/*    all the same).                                                         */
/*    rsx_image_hash: img->data is a host or a device pointer (a multiple of */
/*    sample_bytes; ctx, data or out NULL -> RSX_ERR_INVALID_ARG); line_md5  */
/*    (16 dim_y bytes, may be NULL) and out are host pointers.  With a       */
/*    device pointer nothing but the 16 dim_y + 32 bytes crosses the link.   */
/*    One host call in rsx_ctx_host_calls.  It runs a plan of one job.       */
/* ------------------------------------------------------------------------ */
typedef struct rsx_image_hash_result {
  uint8_t md5[16];
  uint64_t byte_sum;
  uint64_t sample_sum;
} rsx_image_hash_result;

int rsx_image_hash_validate(const rsx_image* img, int32_t sample_bytes);
int rsx_image_hash(rsx_ctx* ctx, const rsx_image* img, int32_t sample_bytes, uint8_t* line_md5,
                   rsx_image_hash_result* out);

/* ------------------------------------------------------------------------ */
/* Device-resident plans (inputs/outputs already in HBM).                    */
/*                                                                           */
/* A plan is "validate + size scratch + upload tables once, launch many".   */
/* `in_dev`/`out_dev` are device base pointers; each job addresses           */
/* [in_offset, in_offset+in_bytes) of the input and an image view starting  */
/* `img_offset` bytes into the output.  `stream` is a hipStream_t (may be    */
/* NULL = the context's stream).  run() only enqueues; results() blocks on   */
/* the stream, then reports per-job status / consumed byte counts.           */
/* The context's stream is hipStreamNonBlocking: with stream == NULL a run   */
/* is queued behind the work the caller has put on the NULL stream so far    */
/* (an event wait); a caller who passes a stream orders the run himself --   */
/* in_dev must be final and out_dev free on THAT stream.                     */
/* ------------------------------------------------------------------------ */
typedef struct rsx_plan rsx_plan;

typedef struct rsx_unpack_job {
  rsx_unpack_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_unpack_job;

typedef struct rsx_unpack_variant_job {
  rsx_unpack_variant_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_unpack_variant_job;

typedef struct rsx_ljpeg_job {
  rsx_ljpeg_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_ljpeg_job;

typedef struct rsx_cr2_job {
  rsx_cr2_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_cr2_job;

typedef struct rsx_nikon_job {
  rsx_nikon_desc desc; /* desc.curve: host pointer, copied at plan creation */
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_nikon_job;

typedef struct rsx_pentax_job {
  rsx_pentax_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_pentax_job;

/* in_offset / img_offset address the subsampled input image and the interpolated
 * output image inside the plan's input / output buffers */
typedef struct rsx_sraw_job {
  rsx_sraw_desc desc;
  uint64_t in_offset;
  uint64_t img_offset;
  rsx_image in;  /* .data ignored */
  rsx_image img; /* .data ignored */
} rsx_sraw_job;

typedef struct rsx_hasselblad_job {
  rsx_hasselblad_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_hasselblad_job;

typedef struct rsx_samsung_v1_job {
  rsx_samsung_v1_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_samsung_v1_job;

typedef struct rsx_samsung_v2_job {
  rsx_samsung_v2_desc desc;
  uint64_t in_offset; /* multiple of 16: the rows start at 16-byte boundaries of the data */
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_samsung_v2_job;

typedef struct rsx_sony_arw1_job {
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_sony_arw1_job;

/* strip offsets are relative to in_offset; jobs of different geometry may share a plan */
typedef struct rsx_phase_one_job {
  const rsx_phase_one_strip* strips; /* host pointer, copied at plan creation */
  int32_t n_strips;
  int32_t reserved;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_phase_one_job;

/* row y of a job starts at in_offset + y dim_x; its table is copied at plan creation */
typedef struct rsx_sony_arw2_job {
  rsx_sony_arw2_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_sony_arw2_job;

/* jobs of different versions, depths and geometries may share a plan; any in_offset, any
 * even pitch_bytes >= 2 dim_x and any even img_offset */
typedef struct rsx_panasonic_job {
  rsx_panasonic_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_panasonic_job;

/* row offsets are relative to in_offset; jobs of different geometry may share a plan; any
 * in_offset, any even pitch_bytes >= 2 dim_x and any even img_offset.  The plan owns a scratch
 * plane of dim_y x roundUp(dim_x, 16) 16-bit values per job. */
typedef struct rsx_samsung_v0_job {
  const uint32_t* row_offsets; /* host pointer, copied at plan creation */
  int32_t n_offsets;
  int32_t reserved;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_samsung_v0_job;

/* jobs of both splits, both flags and different geometries may share a plan; any in_offset, any
 * even pitch_bytes >= 2 dim_x and any even img_offset.  The plan owns a list of min(bad_cap,
 * dim_x dim_y) entries per job with zero_is_bad. */
typedef struct rsx_panasonic_v4_job {
  rsx_panasonic_v4_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
  uint32_t bad_cap;
  uint32_t reserved;
} rsx_panasonic_v4_job;

/* row y of a job starts at in_offset + 3 y dim_x; its table is copied at plan creation.  Jobs of
 * different geometry, white balance and table may share a plan; any in_offset, any even
 * pitch_bytes >= 6 dim_x and any even img_offset */
typedef struct rsx_nikon_snef_job {
  rsx_nikon_snef_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_nikon_snef_job;

/* one image's corrections (section 3n), in place: the pass reads and writes the plan's OUTPUT
 * buffer (rsx_plan_run's in_dev is ignored and may equal out_dev), so a caller runs its Phase One
 * plan and then this one on the same buffer and stream.  Jobs of different geometry and different
 * lists may share a plan; img_offset and pitch_bytes even.  Payloads and curves are copied at plan
 * creation.  Because the work is in place a plan never runs a part of its jobs: a job that fails
 * rsx_iiq_correct_validate fails the creation with that status. */
typedef struct rsx_iiq_correct_job {
  rsx_iiq_corr corr;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_iiq_correct_job;

/* one image's opcode list and look-up (section 4d), in place: the pass reads and writes the plan's
 * OUTPUT buffer (rsx_plan_run's in_dev is ignored and may equal out_dev), so a caller runs its
 * decode plan and then this one on the same buffer and stream.  Jobs of different geometry, lists
 * and tables, uint16 and F32, may share a plan; img_offset a multiple of the sample size.  The
 * list and the table are parsed and copied at plan creation.  Because the work is in place a plan
 * never runs a part of its jobs: a job that rsx_dng_post_validate refuses (RSX_ERR_IO included)
 * fails the creation with that status.  The plan owns min(bad_cap, pixels the job's
 * FixBadPixelsConstant opcodes look at) hit entries per job; a job whose hits exceed them reports
 * RSX_ERR_UNSUPPORTED in rsx_plan_results, its image is complete. */
typedef struct rsx_dng_post_job {
  rsx_dng_post_desc desc;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
  uint32_t bad_cap;
  uint32_t reserved;
} rsx_dng_post_job;

/* one image's bad-pixel stage (section 5), in place on the plan's OUTPUT buffer at img_offset (a
 * multiple of the sample size), so it runs behind a decode plan on the same buffer and stream.
 * The positions, n_positions of them, are read from the plan's INPUT buffer at in_offset (a
 * multiple of 4) by every run; map_in (host memory, may be NULL; map_pitch as in section 5) is
 * copied at plan creation.  Jobs of different geometry, CFA or not, uint16 and F32, may share a
 * plan.  A job the image checks or the map checks of rsx_bad_pixels_validate refuse fails the
 * creation with that status.  The positions are checked on the device: one outside the image
 * makes the job RSX_ERR_INVALID_ARG in rsx_plan_results and leaves its image untouched.  A job
 * without positions and without map_in does nothing.  The plan owns both maps of every job. */
typedef struct rsx_bad_pixels_job {
  uint64_t in_offset;
  uint32_t n_positions;
  uint32_t map_pitch;
  const uint8_t* map_in;
  int32_t is_f32;
  int32_t reserved;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_bad_pixels_job;

/* one image's black/white scaling (section 6), in place on the plan's OUTPUT buffer at img_offset
 * (a multiple of the sample size); the input buffer is not read.  The areas are copied at plan
 * creation.  Jobs of different geometry and variant may share a plan.  A job rsx_scale_validate
 * refuses fails the creation with that status; what only the image can decide (section 6) makes
 * the job RSX_ERR_UNSUPPORTED in rsx_plan_results and leaves its image untouched.  The plan owns
 * the histograms and the generator checkpoints of its jobs. */
typedef struct rsx_scale_job {
  rsx_scale_desc desc;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_scale_job;

/* one VC-5 tile (section 4c): band offsets count from in_offset; the code book and the log table
 * are copied at plan creation.  Jobs of different geometry, book and table may share a plan; any
 * in_offset, any even pitch_bytes >= 2 dim_x and any even img_offset.  The band decode loads a
 * chunk as the aligned dwords that hold a byte of it: up to 3 bytes in front of the chunk's first
 * byte and up to 3 behind its last one are read (and ignored), never a dword without a byte of
 * the chunk -- so the input allocation must begin and end on a 4-byte boundary of the address
 * space, which every hipMalloc allocation does.  The plan owns the band storage of all its jobs
 * (about 7 bytes a pixel) */
typedef struct rsx_vc5_job {
  rsx_vc5_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_vc5_job;

/* one tile of a deflate DNG (section 4b): geometry in samples, as in rsx_dng_deflate_tile; any
 * in_offset, img_offset and pitch_bytes multiples of 4.  The plan owns the inflated bytes of all
 * its jobs (dstLen each, rounded up to 16); more than 1 GiB of them: RSX_ERR_UNSUPPORTED at
 * creation.  job_consumed = the stream's length up to and including the Adler-32. */
typedef struct rsx_dng_deflate_job {
  rsx_dng_deflate_desc desc;
  uint32_t tile_w, tile_h;
  uint32_t off_x, off_y, width, height;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_dng_deflate_job;

/* the tiles of one lossy-JPEG DNG image (section 4e).  The headers, the tables and the restart
 * markers are read from the HOST bytes of `tiles` while the plan is made; a run expects the same
 * bytes of tile t at in_offsets[t] of its input.  The plan owns the component planes of all its
 * tiles (whole MCUs); more than 1 GiB of them: RSX_ERR_UNSUPPORTED at creation.  The job's status
 * is RSX_ERR_TILE_ERRORS if a tile failed; rsx_dng_jpeg_plan_tile_status has the tiles'. */
typedef struct rsx_dng_jpeg_job {
  int32_t n_tiles;
  const rsx_dng_jpeg_tile* tiles;
  const uint64_t* in_offsets;
  uint64_t img_offset; /* a multiple of 2 */
  rsx_image img;       /* .data ignored */
} rsx_dng_jpeg_job;

/* one compressed RAF frame (section 3u); the strip offsets of `desc` are relative to in_offset.
 * Jobs of both types, both depths and different geometries may share a plan: all their strips go
 * into one launch.  Any in_offset, any even pitch_bytes >= 2 dim_x and any even img_offset. */
typedef struct rsx_fuji_job {
  rsx_fuji_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_fuji_job;

int rsx_fuji_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_fuji_job* jobs, rsx_plan** out_plan);
/* Fuji plans, after rsx_plan_results: the statuses of the strips of job `job` of the last run
 * (blocks_in_row entries).  RSX_ERR_INVALID_ARG for another plan, a refused job or before a run. */
int rsx_fuji_plan_strip_status(rsx_plan* plan, int job, int32_t* strip_status);

/* one compressed ORF frame (section 3v).  Jobs of different geometry may share a plan: one
 * wavefront walks each job's bits, four reconstruct its planes.  Any in_offset, any even
 * pitch_bytes >= 2 dim_x and any even img_offset. */
typedef struct rsx_olympus_job {
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_olympus_job;

int rsx_olympus_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_olympus_job* jobs,
                            rsx_plan** out_plan);
/* Olympus plans, after rsx_plan_results (which returns the status of the lowest-numbered failing
 * job): the status of job `job` of the last run.  RSX_ERR_INVALID_ARG for another plan or before
 * a run's results. */
int rsx_olympus_plan_job_status(rsx_plan* plan, int job, int32_t* status);

/* one Kodak DCR frame (section 3w); its table is copied at plan creation.  Jobs of different
 * geometry, depth and table may share a plan: the frames' successor maps are made side by side and
 * all their segments go into one launch.  Any in_offset, any even pitch_bytes >= 2 dim_x and any
 * even img_offset.  Only the first min(in_bytes, what the image can consume) bytes are read.  The
 * plan owns 6 bytes of maps per byte it reads.  rsx_plan_results gives every job its own status;
 * a failing job does not disturb the others. */
typedef struct rsx_kodak_job {
  rsx_kodak_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_kodak_job;

int rsx_kodak_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_kodak_job* jobs,
                          rsx_plan** out_plan);

/* one Canon CRW frame (section 3x).  The scan and the low bits are two ranges of the run's input
 * buffer (low_bytes is ignored without low bits).  Jobs of different geometry and table may share
 * a plan; the windows of all their scans are parsed side by side.  Any in_offset and low_offset,
 * any even pitch_bytes >= 2 dim_x and any even img_offset.  The plan owns about 1.3 bytes per
 * byte of scan it reads.  rsx_plan_results gives every job its own status; a failing job does
 * not disturb the others.  Job results report 0 bytes consumed. */
typedef struct rsx_crw_job {
  rsx_crw_desc desc;
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t low_offset;
  uint64_t low_bytes;
  uint64_t img_offset;
  rsx_image img; /* .data ignored */
} rsx_crw_job;

int rsx_crw_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_crw_job* jobs, rsx_plan** out_plan);

/* After rsx_plan_results: how job `job` of the last run was parsed.  stats[0] the windows of its
 * scan, stats[1] the most rounds a window took to settle its segments, stats[2] the last of the
 * speculative rounds over the windows in which a window's head still changed (0: the first pass
 * had them right), stats[3] != 0 if the settling kernel had to re-parse a window.  The number of
 * speculative rounds is read from RSX_CRW_SPEC_ROUNDS when the context is created (default 4; 0
 * leaves every window behind the first to the settling kernel; values above 32 count as 32).  The result of a run does not
 * depend on it. */
int rsx_crw_plan_stats(rsx_plan* plan, int job, uint32_t stats[4]);

/* one SuperCCD rotation (section 3y).  in_offset / img_offset address the uncropped source image
 * in the run's input buffer and the rotated image in its output buffer (both even; any even
 * pitches; the two buffers may be one allocation as long as the images do not overlap).  Jobs of
 * different geometry and layout share the plan's one launch.  A job rsx_raf_rotate_validate
 * refuses has that status in rsx_plan_results and its image is untouched. */
typedef struct rsx_raf_rotate_job {
  rsx_raf_rotate_desc desc;
  uint64_t in_offset;
  uint64_t img_offset;
  rsx_image in;  /* .data ignored */
  rsx_image img; /* .data ignored */
} rsx_raf_rotate_job;

int rsx_raf_rotate_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_raf_rotate_job* jobs,
                                rsx_plan** out_plan);

/* one Sony SRF frame (section 3z): 2 dim_x dim_y bytes at in_offset (any), the image at an even
 * img_offset with any even pitch_bytes >= 2 dim_x.  Jobs of different geometry and key share the
 * plan's one launch.  A job rsx_sony_srf_validate refuses has that status in rsx_plan_results and
 * its image is untouched.  Job results report 0 bytes consumed. */
typedef struct rsx_sony_srf_job {
  uint64_t in_offset;
  uint64_t in_bytes;
  uint64_t img_offset;
  uint32_t key;
  uint32_t reserved;
  rsx_image img; /* .data ignored */
} rsx_sony_srf_job;

int rsx_sony_srf_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_sony_srf_job* jobs,
                             rsx_plan** out_plan);

/* one image hash (section 4g): rsx_plan_run(plan, images_base, outputs_base, stream).  The image
 * lies at img_offset (a multiple of sample_bytes, as images_base and the pitch are) in the run's
 * input buffer.  Into the run's output buffer (outputs_base a multiple of 16) go the 16 dim_y bytes
 * of the line digests at lines_offset (a multiple of 16) and the 32-byte rsx_image_hash_result at
 * result_offset (a multiple of 8).  The two buffers may be one allocation as long as nothing
 * overlaps.  Jobs of any mix of geometry and sample size share the plan's two launches, and their
 * number is bounded by no grid axis.  A job rsx_image_hash_validate refuses (or whose offsets are
 * off their grids: RSX_ERR_INVALID_ARG) has that status in rsx_plan_results and its outputs are
 * untouched.  Job results report 0 bytes consumed.  The plan is stream-ordered: it can run right
 * behind a decode plan on the same stream and buffer without a host wait. */
typedef struct rsx_image_hash_job {
  uint64_t img_offset;
  uint64_t lines_offset;
  uint64_t result_offset;
  int32_t sample_bytes;
  int32_t reserved;
  rsx_image img; /* .data ignored */
} rsx_image_hash_job;

int rsx_image_hash_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_image_hash_job* jobs,
                               rsx_plan** out_plan);

int rsx_dng_jpeg_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dng_jpeg_job* jobs,
                             rsx_plan** out_plan);
/* After rsx_plan_results: the n_tiles statuses of job `job` of the last run.
 * RSX_ERR_INVALID_ARG for another plan or a job out of range. */
int rsx_dng_jpeg_plan_tile_status(rsx_plan* plan, int job, int32_t* tile_status);
int rsx_unpack_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_unpack_job* jobs,
                           rsx_plan** out_plan);
/* F32 images: same job structure, img describes 4-byte samples */
int rsx_unpack_f32_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_unpack_job* jobs,
                               rsx_plan** out_plan);
int rsx_unpack_variant_plan_create(rsx_ctx* ctx, int n_jobs,
                                   const rsx_unpack_variant_job* jobs,
                                   rsx_plan** out_plan);
int rsx_ljpeg_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_ljpeg_job* jobs,
                          rsx_plan** out_plan);
int rsx_cr2_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_cr2_job* jobs,
                        rsx_plan** out_plan);
/* (jobs with split != 0 cost one host round trip per run: the second table
 * starts at a bit position only known once the first part is decoded) */
int rsx_nikon_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_nikon_job* jobs,
                          rsx_plan** out_plan);
int rsx_pentax_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_pentax_job* jobs,
                           rsx_plan** out_plan);
int rsx_samsung_v1_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_samsung_v1_job* jobs,
                               rsx_plan** out_plan);
int rsx_samsung_v2_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_samsung_v2_job* jobs,
                               rsx_plan** out_plan);
int rsx_sraw_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_sraw_job* jobs,
                         rsx_plan** out_plan);
int rsx_hasselblad_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_hasselblad_job* jobs,
                               rsx_plan** out_plan);
int rsx_sony_arw1_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_sony_arw1_job* jobs,
                              rsx_plan** out_plan);
int rsx_phase_one_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_phase_one_job* jobs,
                              rsx_plan** out_plan);
int rsx_sony_arw2_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_sony_arw2_job* jobs,
                              rsx_plan** out_plan);
int rsx_panasonic_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_panasonic_job* jobs,
                              rsx_plan** out_plan);
int rsx_samsung_v0_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_samsung_v0_job* jobs,
                               rsx_plan** out_plan);
int rsx_panasonic_v4_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_panasonic_v4_job* jobs,
                                 rsx_plan** out_plan);
int rsx_nikon_snef_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_nikon_snef_job* jobs,
                               rsx_plan** out_plan);
int rsx_dng_deflate_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dng_deflate_job* jobs,
                                rsx_plan** out_plan);
int rsx_vc5_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_vc5_job* jobs, rsx_plan** out_plan);
int rsx_iiq_correct_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_iiq_correct_job* jobs,
                                rsx_plan** out_plan);
int rsx_dng_post_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dng_post_job* jobs,
                             rsx_plan** out_plan);
/* DNG post plans: the verdict, the crop and the count of job `job` (any time after creation;
 * n_bad counts the FixBadPixelsConstant hits of the last run once rsx_plan_results has run), and,
 * after rsx_plan_results, its bad-pixel positions in the reference's order with the contract of
 * rsx_panasonic_v4_plan_bad_pixels. */
int rsx_dng_post_plan_result(rsx_plan* plan, int job, rsx_dng_post_result* out);
int rsx_dng_post_plan_bad_pixels(rsx_plan* plan, int job, uint32_t* out, uint32_t cap,
                                 uint64_t* n_bad);
int rsx_bad_pixels_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_bad_pixels_job* jobs,
                               rsx_plan** out_plan);
/* Bad-pixel plans, after rsx_plan_results: the counts of job `job` of the last run.
 * RSX_ERR_INVALID_ARG for another plan, a job out of range or before results. */
int rsx_bad_pixels_plan_result(rsx_plan* plan, int job, rsx_bad_pixels_result* out);
int rsx_scale_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_scale_job* jobs, rsx_plan** out_plan);
/* Scaling plans, after rsx_plan_results: the levels and the verdict of job `job` of the last run
 * (zero for a refused job).  RSX_ERR_INVALID_ARG for another plan, a job out of range or before
 * results. */
int rsx_scale_plan_result(rsx_plan* plan, int job, rsx_scale_result* out);
/* After rsx_plan_results of a VC-5 plan: per band of job `job` ([channel][subband], 40 entries
 * each; any may be NULL) its status, and for the high-pass bands the 128-Kbit windows the band
 * decode walked and the parse rounds it took over all of them (a round is one parse of every
 * segment of a window; a window whose guessed entries were all right takes one). */
int rsx_vc5_plan_bands(rsx_plan* plan, int job, int32_t* band_status, uint32_t* windows,
                       uint32_t* rounds);
/* Enqueue one pass of the plan on `stream`. */
int rsx_plan_run(rsx_plan* plan, const void* in_dev, void* out_dev,
                 void* stream);
/* Wait for the last run and fetch per-job results.  `job_status` and
 * `job_consumed` may be NULL.  Returns RSX_OK iff every job is RSX_OK. */
int rsx_plan_results(rsx_plan* plan, int32_t* job_status,
                     uint32_t* job_consumed);
/* Panasonic V4 plans, after rsx_plan_results: the zero pixels of job `job` of the last run,
 * ascending, into `out` (`cap` entries; NULL with cap 0 is allowed), *n_bad (may be NULL) = the
 * exact count.  RSX_ERR_UNSUPPORTED when the count exceeds `cap` or the job's bad_cap (`out` is
 * not written), RSX_ERR_INVALID_ARG for another plan, a refused job or before results. */
int rsx_panasonic_v4_plan_bad_pixels(rsx_plan* plan, int job, uint32_t* out, uint32_t cap,
                                     uint64_t* n_bad);
/* Name of the dominant kernel of this plan and the average duration (ms) of
 * its launches since the previous call.  Unpack and sRaw plans: the kernel
 * stamps the device's wall clock on entry and exit (first entry to last exit of
 * a launch; up to 64 launches between two calls, further ones go untimed) and a
 * timed launch queues nothing besides the kernel.  The other plans: hipEvents
 * recorded on the launch stream.  Timing is off by default; enable
 * with rsx_plan_set_timing(plan, 1).  Returns RSX_OK, or RSX_ERR_INVALID_ARG
 * if timing is disabled / no launches happened. */
int rsx_plan_set_timing(rsx_plan* plan, int enable);
int rsx_plan_kernel_time(rsx_plan* plan, const char** kernel_name,
                         double* avg_ms, int* n_launches);
/* LJPEG-family plans run a sequence of kernels.  With timing enabled an event is
 * recorded after every launch of a run (on the launch stream), and
 * rsx_plan_kernel_time() names the kernel with the largest total.  This call
 * returns the whole table -- up to `cap` kernel names with their average
 * duration per run (ms) over the timed runs since timing was enabled -- so that
 * the dominant kernel can be checked rather than believed.  *n_kernels = entries
 * the plan has (may exceed cap), *n_runs = runs averaged over. */
int rsx_plan_kernel_table(rsx_plan* plan, int cap, const char** names, double* avg_ms,
                          int* n_kernels, int* n_runs);
void rsx_plan_destroy(rsx_plan* plan);

/* ------------------------------------------------------------------------ */
/* 7. Writers: BitVacuumer* and PrefixCodeVectorEncoder                      */
/*    The write direction of src/librawspeed: bitstreams/BitVacuumer.h with  */
/*    BitVacuumerLSB.h, BitVacuumerMSB.h, BitVacuumerMSB16.h,                */
/*    BitVacuumerMSB32.h and BitVacuumerJPEG.h, and codes/                   */
/*    PrefixCodeVectorEncoder.h over codes/AbstractPrefixCodeEncoder.h.  The */
/*    reference has no call site for them in its decoders (its benchmarks    */
/*    and fuzzers use them): what binds these calls is a writer, a caller    */
/*    who holds a decoded image on the device and wants it back as a packed  */
/*    strip or as lossless-JPEG tiles (the raw-to-DNG direction).            */
/*                                                                           */
/*    7a. Packed integers: the inverse of decodePackedInt.  The descriptor   */
/*    is rsx_unpack_desc with the reader's meaning: rows crop_y .. crop_y +  */
/*    crop_h - 1 of the image become one continuous stream; each row gives   */
/*    crop_w cpp samples of bits_per_pixel bits read from column 0 (the      */
/*    reader ignores crop_x, and so does the writer) followed by             */
/*    input_pitch_bytes - row_bytes zero bytes; the order is LSB, MSB, MSB16 */
/*    or MSB32 with the word addressing of SURVEY.md A.1.  A sample's bits   */
/*    above bits_per_pixel are dropped: BitStreamCache::push does not mask,  */
/*    so this is the one deliberate difference from handing put an oversized */
/*    value.  Tail: BitVacuumer::flush pads with zero bits to a whole 32-bit */
/*    chunk, so roundUp(crop_h pitch, 4) bytes are written (bytes_written)   */
/*    of which crop_h pitch are the stream (stream_bytes).  Validation: the  */
/*    geometry checks of rsx_unpack_validate in its order; then crop_y +     */
/*    crop_h > dim_y, an odd image pitch or one shorter than its samples,    */
/*    and out_cap < roundUp(crop_h pitch, 4) -> RSX_ERR_INVALID_ARG.         */
/*    Integer images only: at the reader's check of bits_per_pixel, 17..32   */
/*    (the widths only an F32 image has) get RSX_ERR_UNSUPPORTED; anything   */
/*    else outside 1..16 RSX_ERR_INVALID_ARG as the reader's does.           */
/*    Image and output are both host pointers or both device pointers.       */
/* ------------------------------------------------------------------------ */
typedef struct rsx_encode_pack_result {
  uint64_t bytes_written; /* roundUp(crop_h pitch, 4) */
  uint64_t stream_bytes;  /* crop_h pitch */
} rsx_encode_pack_result;

int rsx_encode_pack_validate(const rsx_unpack_desc* d, const rsx_image* img, size_t out_cap);
int rsx_encode_pack_u16(rsx_ctx* ctx, const rsx_unpack_desc* d, const rsx_image* img, uint8_t* out,
                        size_t out_cap, rsx_encode_pack_result* bytes);

/* A plan's input buffer holds images and its output buffer holds streams: the image of a job lies
 * at img_offset (even) of the input, its stream goes to out_offset (any) of the output, at most
 * out_cap bytes of it.  Nothing outside [out_offset, out_offset + bytes_written) is touched.  Jobs
 * of any geometry and order share the plan's one launch.  Results report bytes_written as the
 * bytes consumed. */
typedef struct rsx_encode_pack_job {
  rsx_unpack_desc desc;
  uint32_t reserved;
  uint64_t img_offset;
  uint64_t out_offset;
  uint64_t out_cap;
  rsx_image img; /* .data ignored */
} rsx_encode_pack_job;

int rsx_encode_pack_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_encode_pack_job* jobs,
                                rsx_plan** out_plan);

/* 7b. Lossless JPEG scan: the inverse of LJpegDecompressor::decode.  The descriptor is
 * rsx_ljpeg_desc as it stands: a stream written for a descriptor decodes under that descriptor.
 * Accepted is the subset in which every decoded pixel exists in the image: mcu_h == 1, mcu_w ==
 * n_comp in 1..4, frame_w mcu_w == cpp tile_w, frame_h == tile_h, the tile inside the image,
 * rows_per_restart_interval >= 1 (a value >= tile_h means no markers).  rsx_encode_ljpeg_validate
 * returns, in this order, what rsx_ljpeg_validate returns for the descriptor, then
 * RSX_ERR_UNSUPPORTED for MCU 2x2, a frame wider or taller than the tile or a trailing partial
 * MCU, then RSX_ERR_INVALID_ARG for an odd image pitch or one shorter than its row.
 * Per sample: predictor 1 as LJpegDecompressor reconstructs it (the left sample of the component;
 * for the first MCU of a row the first MCU of the row above; in the first row of the tile or of a
 * restart interval init_pred[c]); d = int16(uint16(x - pred)); (diff, ssss) = reduce(d) of
 * AbstractPrefixCodeEncoder.h:48-58, -32768 giving ssss 16; the symbol word is the code followed
 * by the ssss low bits, for ssss 16 the code alone, or with fix_dng_bug16 the code and 16 zero
 * bits.  Every data byte FF is followed by 00 (BitVacuumerJPEG.h:84-91); between restart intervals
 * the bit stream is closed and FF D0+((i-1)%8) follows (LJpegDecompressor.cpp:288-298).
 * Tail, chosen by `flags`:
 *   RSX_ENCODE_TAIL_JPEG      pad with 1-bits to a byte boundary, a final FF stuffed like any other
 *                             (T.81 F.1.2.3; byte for byte the test writer's stream).  Intervals in
 *                             front of a marker are closed like this in either mode: the
 *                             reference's reader needs the marker at the next byte.
 *   RSX_ENCODE_TAIL_VACUUMER  the last interval ends as BitVacuumerJPEG::flush ends it: zero bits
 *                             up to a whole 32-bit chunk, the stuffing applied to its bytes.
 * Results per job: status, entropy bytes written, symbol bits.  Data-dependent statuses: a
 * category the component's table lacks -> RSX_ERR_BAD_HUFFMAN_CODE; a stream that would pass
 * out_cap -> RSX_ERR_INPUT_OVERFLOW; in both cases 0 bytes are reported and the job's output range
 * may hold anything up to out_cap but nothing past it.  out_cap below the bound is no error at
 * validation.  rsx_encode_ljpeg_bound is the host closed form: 4 bytes a sample, doubled for
 * stuffing, plus 2 a marker, plus 8 (0 for a descriptor the validation refuses). */
#define RSX_ENCODE_TAIL_JPEG 0
#define RSX_ENCODE_TAIL_VACUUMER 1

typedef struct rsx_encode_result {
  int32_t status;
  int32_t reserved;
  uint64_t bytes;       /* entropy bytes written (0 unless status is RSX_OK) */
  uint64_t symbol_bits; /* code and difference bits, without padding, stuffing and markers */
} rsx_encode_result;

int rsx_encode_ljpeg_validate(const rsx_ljpeg_desc* d, const rsx_image* img);
uint64_t rsx_encode_ljpeg_bound(const rsx_ljpeg_desc* d, const rsx_image* img);
/* img->data and out: both host pointers or both device pointers; result: host.  Returns the
 * job's status. */
int rsx_encode_ljpeg(rsx_ctx* ctx, const rsx_ljpeg_desc* d, const rsx_image* img, uint32_t flags,
                     uint8_t* out, size_t out_cap, rsx_encode_result* result);

/* Jobs of different geometry and tables share a plan: the tiles of a DNG are the jobs of one
 * plan.  rsx_plan_results reports per-job status and the bytes written as bytes consumed;
 * rsx_encode_ljpeg_plan_result, after it, the whole result of job `job` of the last run.
 * Nothing beyond the written bytes of a job is touched. */
typedef struct rsx_encode_ljpeg_job {
  rsx_ljpeg_desc desc;
  uint32_t flags; /* RSX_ENCODE_TAIL_* */
  uint32_t reserved;
  uint64_t img_offset;
  uint64_t out_offset;
  uint64_t out_cap;
  rsx_image img; /* .data ignored */
} rsx_encode_ljpeg_job;

int rsx_encode_ljpeg_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_encode_ljpeg_job* jobs,
                                 rsx_plan** out_plan);
int rsx_encode_ljpeg_plan_result(rsx_plan* plan, int job, rsx_encode_result* out);

/* Host only: SOI, SOF3, DHT(s), optional DRI and SOS in front of a scan of `entropy_bytes` bytes
 * into hdr_out (*hdr_bytes of them), in the layout of SURVEY.md Appendix C; EOI (FF D9) goes
 * behind the scan and is the caller's to append.  With it a job's bytes become a tile that
 * LJpegDecoder takes.  RSX_ERR_INVALID_ARG: a descriptor the validation refuses, a frame or a
 * restart interval past 65535, hdr_cap too small. */
int rsx_encode_ljpeg_container(const rsx_ljpeg_desc* d, const rsx_image* img, int32_t precision,
                               uint64_t entropy_bytes, uint8_t* hdr_out, size_t hdr_cap,
                               size_t* hdr_bytes);

/* 7c. The difference histogram of a tile and the table made from it.  The histogram is the
 * category of every sample's difference, counted per component: counts[17 c + ssss], 4 x 17
 * 64-bit counts (host memory).  The call takes the descriptor of the encode and ignores its
 * tables (they must still pass the validation).  img->data is a host or a device pointer.
 * rsx_encode_huff_from_histogram (host only) turns 17 counts into a table by T.81 Annex K.2
 * (Figures K.1 - K.4): the all-ones code point reserved, lengths limited to 16.  A category with
 * count 0 is left out; RSX_ENCODE_TABLE_ALL_CATEGORIES gives every absent category of 0..16 a
 * count of 1 first, so that the table also serves other tiles.  RSX_ERR_INVALID_ARG for a
 * histogram without counts. */
#define RSX_ENCODE_TABLE_ALL_CATEGORIES 1
int rsx_encode_ljpeg_histogram(rsx_ctx* ctx, const rsx_ljpeg_desc* d, const rsx_image* img,
                               uint64_t* counts);
int rsx_encode_huff_from_histogram(const uint64_t* counts, uint32_t flags, rsx_huff_table* out);

/* 7d. Floating-point images (RawImageType::F32): the inverse of rsx_unpack_f32 (section 1a) and
 * the width an image needs.  All names begin with rsx_fpwrite_.
 *
 * Narrowing.  binary32 -> binary16 (16 bits) or binary24 (24 bits) is the inverse of
 * extendBinaryFloatingPoint (common/FloatingPoint.h:109-145) and is defined only where widening
 * the result gives the sample back as a 32-bit pattern: no rounding, no clamping.  The rule is
 * bitwise: -0, the infinities and NaNs whose low 23 - FRAC fraction bits are zero have a narrow
 * pattern; a binary32 normal in the narrow format's subnormal range has one iff the bits shifted
 * out are zero; a binary32 subnormal other than +-0 has none.  A sample without one is inexact.
 *
 * rsx_fpwrite_fit reports for each window of an F32 image the least of 16 / 24 / 32 under which
 * every sample of the window narrows exactly: what a DNG writer sets BitsPerSample from.  A window
 * counts samples (cpp folded in: x in [0, dim_x cpp)).  img->data is a host or a device pointer;
 * all windows share one launch.  RSX_ERR_INVALID_ARG: no window, a window empty or outside the
 * image, dim_x or dim_y < 1, cpp outside 1..4, a pitch that is no multiple of 4 or shorter than a
 * row, data off the 4-byte grid.
 *
 * rsx_fpwrite_pack.  The descriptor is rsx_unpack_desc with the meaning rsx_unpack_f32 gives it:
 * 32 bits is copyPixels (crop_x counts pixels), 16 and 24 bits are MSB or LSB order (whole bytes:
 * big- or little-endian samples) and crop_x is a SAMPLE offset as decodePackedFP has it; each row
 * gives crop_w cpp samples followed by input_pitch_bytes - row_bytes zero bytes; the tail follows
 * 7a: roundUp(crop_h pitch, 4) bytes are written.  A stream written for a descriptor unpacks under
 * that descriptor to the same image.  Validation: rsx_unpack_f32_validate's verdicts in its order
 * (of its size checks, the 32-bit one), then dim_x or dim_y < 1, a crop outside the image, an image pitch that is no
 * multiple of 4 or shorter than the samples read, and out_cap < roundUp(crop_h pitch, 4) ->
 * RSX_ERR_INVALID_ARG.  An inexact sample gives the job RSX_ERR_VALUE_RANGE: bytes_written is 0,
 * `inexact` counts such samples, and the job's output range may hold anything up to
 * roundUp(crop_h pitch, 4) bytes but nothing past it.  Image and output are both host pointers or
 * both device pointers. */
typedef struct rsx_fpwrite_window {
  int32_t x, y, w, h; /* samples */
} rsx_fpwrite_window;

int rsx_fpwrite_fit(rsx_ctx* ctx, const rsx_image* img, int n_windows,
                    const rsx_fpwrite_window* windows, int32_t* min_bps_out);

typedef struct rsx_fpwrite_pack_result {
  uint64_t bytes_written; /* roundUp(crop_h pitch, 4); 0 unless the status is RSX_OK */
  uint64_t stream_bytes;  /* crop_h pitch */
  uint64_t inexact;       /* samples without a narrow pattern */
} rsx_fpwrite_pack_result;

int rsx_fpwrite_pack_validate(const rsx_unpack_desc* d, const rsx_image* img, size_t out_cap);
int rsx_fpwrite_pack(rsx_ctx* ctx, const rsx_unpack_desc* d, const rsx_image* img, uint8_t* out,
                     size_t out_cap, rsx_fpwrite_pack_result* result);

/* Jobs as in 7a: the image of a job lies at img_offset (a multiple of 4) of the plan's input
 * buffer, its stream goes to out_offset (any) of the output buffer.  rsx_plan_results reports
 * per-job status and the bytes written as bytes consumed; rsx_fpwrite_pack_plan_result, after it,
 * the whole result of job `job` of the last run. */
typedef struct rsx_fpwrite_pack_job {
  rsx_unpack_desc desc;
  uint32_t reserved;
  uint64_t img_offset;
  uint64_t out_offset;
  uint64_t out_cap;
  rsx_image img; /* .data ignored */
} rsx_fpwrite_pack_job;

int rsx_fpwrite_pack_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_fpwrite_pack_job* jobs,
                                 rsx_plan** out_plan);
int rsx_fpwrite_pack_plan_result(rsx_plan* plan, int job, rsx_fpwrite_pack_result* out);

/* Deflate tiles (compression 8): the inverse of rsx_dng_decompress_deflate (section 4b).  The
 * descriptor is rsx_dng_deflate_desc as it stands; a tile carries the geometry of
 * rsx_dng_deflate_tile, in samples with cpp folded in (predFactor = {1, 2, 4} cpp), and where its
 * stream goes.  The bytes a tile compresses: per row bytesps byte planes of tile_w bytes, most significant
 * first, of the narrow samples (0 outside the window), then b[col] -= b[col - predFactor] from the
 * end of the row down where the row is longer than predFactor.  The stream: CMF 0x78, FLG 0x01 (no
 * FDICT), deflate blocks of RSX_FPWRITE_BLOCK input bytes each (the last one shorter), the
 * big-endian Adler-32 of the bytes.  A block is dynamic-Huffman, or stored when the stored form
 * (padding included) is not longer.  Matches: length 3..258, distance 1..32768, across block
 * boundaries but never before the tile's first byte nor past the block's end.  The stream is a
 * function of the tile's bytes alone: the same from run to run, and byte for byte what the host
 * build of rsx_deflate_core.h writes.
 * Validation: rsx_dng_deflate_validate's verdicts in its order, then a NULL or mixed-side pointer,
 * a tile of 2^28 bytes or more -> RSX_ERR_UNSUPPORTED.  Per tile: an inexact sample ->
 * RSX_ERR_VALUE_RANGE; a stream that would pass out_cap -> RSX_ERR_INPUT_OVERFLOW; in both cases 0
 * bytes are reported and nothing at or past out_cap is touched (nothing is written at all).  The
 * call returns RSX_ERR_TILE_ERRORS if any tile failed.  rsx_fpwrite_deflate_bound is the host
 * closed form: the tile's bytes + 6 a block (3 header bits, up to 7 bits of padding, LEN, NLEN) +
 * 2 + 4; the emit writes single bytes and needs no word padding (0 for a refused tile). */
#define RSX_FPWRITE_BLOCK 16384

typedef struct rsx_fpwrite_deflate_tile {
  uint8_t* out;
  size_t out_cap;
  uint32_t tile_w, tile_h;              /* samples */
  uint32_t off_x, off_y, width, height; /* samples */
} rsx_fpwrite_deflate_tile;

typedef struct rsx_fpwrite_deflate_result {
  int32_t status;
  uint32_t adler;         /* Adler-32 of the tile's bytes */
  uint64_t bytes;         /* of the stream (0 unless status is RSX_OK) */
  uint32_t blocks;        /* deflate blocks */
  uint32_t stored_blocks; /* ... of which stored */
} rsx_fpwrite_deflate_result;

int rsx_fpwrite_deflate_validate(const rsx_dng_deflate_desc* desc,
                                 const rsx_fpwrite_deflate_tile* tile, const rsx_image* img);
uint64_t rsx_fpwrite_deflate_bound(const rsx_dng_deflate_desc* desc,
                                   const rsx_fpwrite_deflate_tile* tile, const rsx_image* img);
/* img->data and every tile's out: all host pointers or all device pointers; results: host */
int rsx_fpwrite_deflate(rsx_ctx* ctx, const rsx_dng_deflate_desc* desc, int n_tiles,
                        const rsx_fpwrite_deflate_tile* tiles, const rsx_image* img,
                        rsx_fpwrite_deflate_result* results);

/* a tile of a plan: the image at img_offset (a multiple of 4) of the run's input buffer, the
 * stream at out_offset of its output buffer.  rsx_plan_results reports per-job status and the
 * stream's bytes as bytes consumed; rsx_fpwrite_deflate_plan_result the whole result. */
typedef struct rsx_fpwrite_deflate_job {
  rsx_dng_deflate_desc desc;
  uint32_t tile_w, tile_h;
  uint32_t off_x, off_y, width, height;
  uint64_t img_offset;
  uint64_t out_offset;
  uint64_t out_cap;
  rsx_image img; /* .data ignored */
} rsx_fpwrite_deflate_job;

int rsx_fpwrite_deflate_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_fpwrite_deflate_job* jobs,
                                    rsx_plan** out_plan);
int rsx_fpwrite_deflate_plan_result(rsx_plan* plan, int job, rsx_fpwrite_deflate_result* out);

/* 7e. Lossy (baseline DCT) JPEG tiles, compression 0x884c: the inverse of section 4e.  All names
 * begin with rsx_dctwrite_.  The stream is byte for byte what libjpeg-turbo's default compressor
 * writes, through Pillow, for save(frame, "JPEG", quality= | qtables=, subsampling=0|1|2,
 * restart_marker_blocks=) with every other option left alone (JDCT_ISLOW, the Huffman tables of
 * Annex K.3, no optimisation, one sequential scan).
 *
 * Input.  The frame is the window (off_x, off_y, width, height) of a uint16 image with cpp 1
 * (grey) or 3 (RGB in, YCbCr stored).  The frame may reach past the image's right and bottom edge
 * (DNG edge tiles are full-size): a frame pixel outside the image is the nearest image pixel.  A
 * sample above 255 is RSX_ERR_VALUE_RANGE for the tile; nothing is clamped.
 *
 * Arithmetic, all integers.  jccolor: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,
 * Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16, Cr = (32768 R - 27439 G - 5329 B + 8421375)
 * >> 16.  Sampling of luma against chroma is (1,1), (2,1) or (2,2); grey is (1,1).  A component of
 * w x h samples (w = ceil(width / h_samp), h = ceil(height / v_samp) for chroma) has
 * ceil(w / 8) x ceil(h / 8) real blocks.  jcsample: chroma sample (x, y), x below 8 ceil(w / 8), is
 * the box over frame columns min(2 x + i, width - 1) and, with y' = min(y, h - 1), frame rows
 * min(v_samp y' + j, height - 1): (a + b + bias) >> 1 with bias 0, 1 alternating by x for (2,1),
 * (a + b + c + d + bias) >> 2 with bias 1, 2 for (2,2).  (Columns are replicated at full
 * resolution, rows at the component's: what libjpeg's expand_right_edge and its padding to a full
 * iMCU row do.)  Luma and unsampled chroma take frame pixel (min(x, width - 1), min(y, height - 1)).
 * jfdctint (CONST_BITS 13, PASS1_BITS 2) on the samples minus 128, rows then columns; coefficient x
 * with table entry q becomes sign(x) ((|x| + 4 q) / (8 q)).
 * A block of an interleaved MCU at or past the component's width or height in blocks is a dummy:
 * 63 zero ACs and the DC of the block before it in the MCU, so its DC difference is 0.
 *
 * Entropy coding: T.81 F.1.2 with Annex K.3's four tables; DC predictors restart at 0 in every
 * restart interval of restart_interval MCUs (0: one interval; the last may be short); every data
 * FF is followed by 00; an interval is closed with 1-bits to a byte (an FF of the padding stuffed
 * like any other); FF D0+(i mod 8) follows interval i but the last, FF D9 the last.
 *
 * Container: SOI, APP0 (JFIF 1.01, units 0, density 1 x 1; only with RSX_DCTWRITE_JFIF), one DQT
 * per table in use (zig-zag order, 8 bits), SOF0 (ids 1, 2, 3; tables 0, 1, 1), one DHT per table
 * (DC0, AC0, then DC1, AC1 for three components), DRI if restart_interval != 0, SOS.  Without APP0
 * the ids still say YCbCr to the reader (section 4e).
 *
 * rsx_dctwrite_validate, in this order: no descriptor or image; an image that cannot hold 16-bit
 * samples (no pixels, cpp < 1, an odd pitch_bytes, pitch_bytes < 2 cpp dim_x); components != cpp;
 * off_x >= dim_x or off_y >= dim_y; width or height 0 or above 65535; restart_interval above
 * 65535; an unknown flag or reserved != 0 (kept for caller-supplied Huffman tables); an entry of a
 * table in use outside 1..255 -> RSX_ERR_INVALID_ARG; then components other than 1 or 3, sampling
 * other than (1,1), (2,1), (2,2), or grey that is not (1,1) -> RSX_ERR_UNSUPPORTED.
 * Per tile of a run: RSX_ERR_VALUE_RANGE (a sample above 255), RSX_ERR_INPUT_OVERFLOW (the stream
 * would pass out_cap); in both cases 0 bytes are reported and nothing of the tile is written.  The
 * call returns RSX_ERR_TILE_ERRORS if any tile failed; the others are written.  Nothing outside
 * a tile's reported bytes is touched, and two runs give the same bytes.
 *
 * rsx_dctwrite_bound is a host closed form (0 for a refused descriptor): the header's bytes
 * + 416 for every block of every MCU (dummies included) + 4 for every interval + 2.  A block is
 * at most 9 + 11 bits of DC and 63 (16 + 10) bits of AC = 1658 bits < 208 bytes, twice that if
 * every byte were FF; an interval adds up to 7 bits of padding, that byte's 00 and its marker.
 *
 * rsx_dctwrite_quality_tables (host only) is jpeg_quality_scaling over Annex K.1's tables with
 * force_baseline, quality 1..100 (else RSX_ERR_INVALID_ARG): what quality= selects. */
#define RSX_DCTWRITE_JFIF 1u

typedef struct rsx_dctwrite_desc {
  uint32_t off_x, off_y, width, height; /* the frame: pixels of the image */
  int32_t components;                   /* 1 or 3, = img->cpp */
  int32_t h_samp, v_samp;               /* luma against chroma */
  uint32_t restart_interval;            /* MCUs; 0: none */
  uint32_t flags;                       /* RSX_DCTWRITE_JFIF */
  uint32_t reserved;                    /* 0: the Huffman tables are Annex K.3's */
  uint16_t qtables[2][64];              /* luma, chroma: natural order, 1..255 */
} rsx_dctwrite_desc;

typedef struct rsx_dctwrite_tile {
  rsx_dctwrite_desc desc;
  uint8_t* out;
  size_t out_cap;
} rsx_dctwrite_tile;

typedef struct rsx_dctwrite_result {
  int32_t status;
  uint32_t reserved;
  uint64_t bytes;       /* SOI..EOI (0 unless status is RSX_OK) */
  uint64_t scan_bytes;  /* behind the SOS segment, up to and without EOI */
  uint64_t symbol_bits; /* Huffman codes and value bits, without padding and stuffing */
} rsx_dctwrite_result;

int rsx_dctwrite_quality_tables(int quality, uint16_t* luma, uint16_t* chroma);
int rsx_dctwrite_validate(const rsx_dctwrite_desc* desc, const rsx_image* img);
uint64_t rsx_dctwrite_bound(const rsx_dctwrite_desc* desc, const rsx_image* img);
/* img->data and every tile's out: all host pointers or all device pointers; results: host.  One
 * upload, one launch sequence, one download; one host call in rsx_ctx_host_calls. */
int rsx_dctwrite(rsx_ctx* ctx, int n_tiles, const rsx_dctwrite_tile* tiles, const rsx_image* img,
                 rsx_dctwrite_result* results);

/* a tile of a plan: the image at img_offset (even) of the run's input buffer, the stream at
 * out_offset (any) of its output buffer; tiles of any geometry share a plan.  A job that
 * rsx_dctwrite_validate refuses keeps that status and writes nothing.  rsx_plan_results reports
 * per-job status and the stream's bytes as bytes consumed; rsx_dctwrite_plan_result, after it, the
 * whole result of job `job` of the last run. */
typedef struct rsx_dctwrite_job {
  rsx_dctwrite_desc desc;
  uint64_t img_offset;
  uint64_t out_offset;
  uint64_t out_cap;
  rsx_image img; /* .data ignored */
} rsx_dctwrite_job;

int rsx_dctwrite_plan_create(rsx_ctx* ctx, int n_jobs, const rsx_dctwrite_job* jobs,
                             rsx_plan** out_plan);
int rsx_dctwrite_plan_result(rsx_plan* plan, int job, rsx_dctwrite_result* out);

/* Measurement aid, not part of the decode path: runs a plain streaming kernel
 * (16-byte loads of in_bytes, 16-byte stores of out_bytes, device pointers) `reps`
 * times on `stream` and returns the average duration in ms, measured with
 * hipEvents on that stream.  bench.py uses it to report the copy ceiling of the
 * device for the read:write mix of an unpack launch next to the vendor peak
 * ("also report a measured device-copy ceiling"). */
int rsx_probe_stream_copy(rsx_ctx* ctx, const void* in_dev, size_t in_bytes,
                          void* out_dev, size_t out_bytes, void* stream, int reps,
                          double* avg_ms);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RSX_H */
