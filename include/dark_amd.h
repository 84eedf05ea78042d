/* dark_amd.h -- C ABI of the MI355X-native BWT compression path that drops in for kvark/dark's
 * src/saca.rs + src/block + src/model + src/entropy.
 *
 * Every entry point names the reference interface it replaces (paths relative to the reference root).
 * Conventions (mirroring the reference's `&mut self` objects):
 *   - a dk_ctx is owned by one host thread and one GPU; it is NOT thread-safe; distinct contexts may run
 *     concurrently on distinct threads / GPUs;
 *   - all functions return DK_OK (0) or a negative DK_E_* code and never unwind or abort across the boundary;
 *     dk_last_error() gives the text of the last failure on that context;
 *   - "host" entry points take caller-owned host pointers valid for the call; "dk_dev_" entry points take
 *     caller-owned DEVICE pointers (hipMalloc'ed on the context's GPU, e.g. torch tensor .data_ptr());
 *   - stream contract of the dk_dev_ entry points: the library works on its own non-blocking HIP stream and synchronises it
 *     before returning, so outputs are complete on return.  It does NOT order its work after the caller's streams: device
 *     INPUTS must be complete (the producing stream synchronised) before the call.  dark_amd/context.py does that for
 *     torch tensors (torch.cuda.current_stream().synchronize());
 *   - n == 0 is an error (the reference panics at src/saca.rs:107); n must be <= dk_capacity();
 *   - there is no CPU fallback: without a GPU dk_ctx_create fails.  Suffix sorting, BWT, DC distances and
 *     the inverse BWT run on the GPU; the adaptive range coder and dc::decode are serial by construction
 *     (every symbol updates the model the next one reads) and run on the host inside this library.
 */
#ifndef DARK_AMD_H
#define DARK_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DK_OK 0
#define DK_E_ARG (-1)        /* null pointer, n == 0, n > capacity, origin out of range ... */
#define DK_E_NOMEM (-2)      /* host or device allocation failed */
#define DK_E_HIP (-3)        /* HIP runtime error (text in dk_last_error) */
#define DK_E_CAPACITY (-4)   /* caller's output buffer is too small */
#define DK_E_MODEL (-5)      /* unknown model id, or the model cannot represent a value at this block size */
#define DK_E_STREAM (-6)     /* corrupt / truncated stream, or a stream the reference format cannot decode */
#define DK_E_INTERNAL (-7)   /* invariant violated (bug) */
#define DK_E_NODEVICE (-8)   /* no usable GPU: this library has no CPU backend */

/* model ids = the -m names of src/main.rs:73-82 */
#define DK_MODEL_DARK 0   /* src/model/dark.rs   (valid for every block size < 2^31) */
#define DK_MODEL_EXP 1    /* src/model/exp.rs    (CLI default; distances truncated to 24 bits: n <= 2^24) */
#define DK_MODEL_YBS 2    /* src/model/ybs.rs    (distances < 2^29) */
#define DK_MODEL_SIMPLE 3 /* src/model/simple.rs (distances < 2^24 + 255) */
#define DK_MODEL_RAWDC 4  /* src/model/raw.rs:12-44 DcOut: 10-byte records instead of a coded stream */
/* Any-byte extension (nothing in the reference corresponds), OR-ed into one of the four coding models above: the stream becomes
 * [u32 LE first_ff][the reference stream, unchanged], first_ff = init[255] = the first position of byte 0xFF in the BWT, or n when the block
 * holds none.  Those four bytes are all the reference's init-table header leaves out (src/block/dc.rs:57,60,73,127), so with the flag EVERY
 * block decodes, a block of nothing but 0xFF included.  The prefix is always there under the flag; out_len, out_cap, dk_last_consumed and the
 * `consumed` of dk_stream_decode count it.  Decoding: in_len < 4 or first_ff > n is DK_E_STREAM.  Every entry point that takes a model_id takes
 * the flag, except dk_model_encode / dk_model_decode (no header there); with those, with DK_MODEL_RAWDC or with an unknown base id: DK_E_MODEL.
 * Without the flag nothing changes.  The DK_RAWMODEL_* ids are a different id space and carry 0xFF already. */
#define DK_MODEL_ANYBYTE 0x100

typedef struct dk_ctx dk_ctx;

/* saca::Constructor::new(max_n) src/saca.rs:351-360 + block::dc::{Encoder,Decoder}::new src/block/dc.rs:30-37,106-115.
 * Allocates the device workspace for blocks of up to max_n bytes on GPU `hip_device` (>= 0). */
int dk_ctx_create(int hip_device, size_t max_n, dk_ctx **out);
/* The two purposes of a context.  DK_CTX_FULL (dk_ctx_create) serves every entry point; its workspace is sized for the suffix sort, about
 * 69.4 x max_n + 64 MiB.  DK_CTX_DECODER serves the inverse path only, in about 14.6 x max_n: the inverse BWT never touches the sort's keys,
 * lists and rank array.  (There is no encoder-only tier: the forward path's L-first route and its fallback share the sort's whole buffer plan.) */
#define DK_CTX_FULL 0
#define DK_CTX_DECODER 1
/* block::dc::Decoder::new / block::raw::Decoder::new (src/block/dc.rs:106-115, src/block/raw.rs): a context that serves the inverse path only.
 * max_n: largest block, and largest pack (sum of its blocks); max_blocks (>= 1, <= DK_PACKED_MAX_BLOCKS): most blocks a packed call may hold
 * (a packed call with more is DK_E_ARG).
 * Served: dk_bwt_inverse, dk_dev_bwt_inverse, dk_block_decode, dk_dev_block_decode, dk_dev_batch_decode, dk_dev_bwt_inverse_packed,
 * dk_dev_packed_decode, dk_raw_block_decode, dk_dc_decode, and dk_capacity, dk_last_error, dk_last_consumed, statistics and profiling -- with
 * the results and return codes of a full context, DK_MODEL_ANYBYTE included.
 * Refused: every entry point that sorts suffixes, builds a BWT, an LCP array or DC arrays or encodes (host, dk_dev_, batch and packed forms), and the
 * dk_dbg_ entries that run the sort layer (dk_dbg_mail_fill and dk_dbg_ws_peek are served): DK_E_ARG, dk_last_error names the entry, nothing
 * is allocated, launched or copied, and the context stays usable. */
int dk_ctx_create_decoder(int hip_device, size_t max_n, size_t max_blocks, dk_ctx **out);
/* DK_CTX_FULL or DK_CTX_DECODER (DK_E_ARG for a null context) */
int dk_ctx_purpose(const dk_ctx *ctx);
/* the workspace dk_ctx_create (DK_CTX_FULL; max_blocks ignored) / dk_ctx_create_decoder would allocate; needs no GPU; 0 for bad arguments */
size_t dk_workspace_bytes(int purpose, size_t max_n, size_t max_blocks);
void dk_ctx_destroy(dk_ctx *ctx);
/* saca::Constructor::capacity src/saca.rs:363-365 */
size_t dk_capacity(const dk_ctx *ctx);
const char *dk_last_error(const dk_ctx *ctx);
/* library / build identification, e.g. "dark_amd 0.1 gfx950" */
const char *dk_version(void);

/* ---- host-pointer entry points ------------------------------------------------------------------------- */
/* saca::Constructor::compute src/saca.rs:368-378: sa_out[0..n) = suffix array of in[0..n)
 * (no sentinel; a suffix that is a prefix of another sorts first). */
int dk_suffix_array(dk_ctx *ctx, const uint8_t *in, size_t n, uint32_t *sa_out);
/* compress::bwt::TransformIterator as driven by src/block/dc.rs:45-50: bwt_out[i] = in[SA[i]-1] (in[n-1] where
 * SA[i]==0), *origin = the i with SA[i]==0.  Known answers src/saca.rs:411-412. */
int dk_bwt_forward(dk_ctx *ctx, const uint8_t *in, size_t n, uint8_t *bwt_out, uint32_t *origin);
/* compress::bwt::decode as driven by src/block/dc.rs:154-156.  DK_E_STREAM when (bwt, origin) is no BWT of any text: the successor
 * table is then a path from origin that is shorter than n plus one or more cycles, whether or not a cycle is ever visited.  DK_OK means
 * all n bytes were written.  On DK_E_STREAM `out` is untouched. */
int dk_bwt_inverse(dk_ctx *ctx, const uint8_t *bwt, size_t n, uint32_t origin, uint8_t *out);
/* compress::bwt::dc::encode + EncodeIterator as driven by src/block/dc.rs:52,82-85, compacted: one entry per run
 * of the BWT, in position order.  init[s] = first position of s, or n if absent.  dist/sym/rank hold up to n
 * entries (rank = Context.last_rank, may be NULL); *m = number of entries. */
int dk_dc_encode(dk_ctx *ctx, const uint8_t *bwt, size_t n, uint32_t init[256],
                 uint32_t *dist, uint8_t *sym, uint8_t *rank, size_t *m);
/* compress::bwt::dc::decode as driven by src/block/dc.rs:146-150 (host, serial).  *consumed (may be NULL) = number of
 * distances read. */
int dk_dc_decode(dk_ctx *ctx, const uint32_t init[256], const uint32_t *dist, size_t m,
                 uint8_t *bwt_out, size_t n, size_t *consumed);
/* block::Encoder::encode for block::dc::Encoder<M> src/block/dc.rs:41-91.  Output = the coded stream WITHOUT the
 * u32 n header that src/main.rs:102 writes in front of it. */
int dk_block_encode(dk_ctx *ctx, int model_id, const uint8_t *in, size_t n,
                    uint8_t *out, size_t out_cap, size_t *out_len);
/* block::Decoder::decode for block::dc::Decoder<M> src/block/dc.rs:119-160 */
int dk_block_decode(dk_ctx *ctx, int model_id, const uint8_t *in, size_t in_len, size_t n, uint8_t *out);
/* block::raw::{Encoder,Decoder}<M: RawModel> src/block/raw.rs:17-105: SA -> BWT, then origin as four symbols (bits 31..24 first,
 * src/block/raw.rs:48-51) and every BWT byte through the RawModel.  RawModels of the reference:
 *   DK_RAWMODEL_OUT  model::raw::Out src/model/raw.rs:46-76: every symbol is appended to ./out.raw, nothing reaches the coder.  Here the
 *                    symbols come back in `dump` (n + 4 bytes) and `out` receives what the idle coder's finish() writes (4 zero bytes).
 *                    Decoding "is not supported" in the reference (raw.rs:71-75 returns symbol 0 for everything): n zero bytes, DK_OK.
 *   DK_RAWMODEL_BBB  model::bbb::Model src/model/bbb.rs: the BWT bytes are coded bit by bit into `out` (dump is not used, may be NULL).
 *                    The model's structure follows bbb.rs; its gates (compress::entropy::ari::apm::Gate, not in the reference tree)
 *                    are restated after the in-repo analogue etc/bbb/main.cpp:348-460 -- PARITY UNPINNED: a stream made here decodes
 *                    here; compatibility with the Rust crate's bytes is not claimed. */
#define DK_RAWMODEL_OUT 0
#define DK_RAWMODEL_BBB 1
int dk_raw_block_encode(dk_ctx *ctx, int raw_model, const uint8_t *in, size_t n, uint8_t *out, size_t out_cap, size_t *out_len,
                        uint8_t *dump, size_t dump_cap, size_t *dump_len);
int dk_raw_block_decode(dk_ctx *ctx, int raw_model, const uint8_t *in, size_t in_len, size_t n, uint8_t *out);
/* Bytes of `in` the last dk_block_decode / dk_dev_block_decode on this context consumed (= the length the encoder wrote:
 * 4 priming bytes + one per renormalisation shift).  Lets a caller walk concatenated [u32 n][stream] records -- the
 * multi-block extension of the single-block file of src/main.rs:70,102. */
size_t dk_last_consumed(const dk_ctx *ctx);
/* Properties of the block the last dk_block_encode / dk_dev_block_encode on this context coded (0 after any other call):
 *   DK_FLAG_HAS_FF         the block contains byte 0xFF.  The stream is bit-exact with the reference's, and like the reference's it
 *                          cannot be decoded: the init-table header never transmits symbol 0xFF (src/block/dc.rs:57,60,73,127).
 *                          A front end should refuse or warn (dark_amd/cli.py does) instead of writing an archive that is lost,
 *                          or code the block with DK_MODEL_ANYBYTE (the flag is reported with it too).
 *   DK_FLAG_SINGLE_SYMBOL  one distinct symbol: the reference's decoder mis-reads `origin` for such a block;
 *                          this library's decoder returns all n bytes. */
#define DK_FLAG_HAS_FF 1u
#define DK_FLAG_SINGLE_SYMBOL 2u
unsigned dk_last_block_flags(const dk_ctx *ctx);

/* ---- device-resident entry points (inputs already in HBM; used by pipelines and by bench.py) ----------------- */
int dk_dev_suffix_array(dk_ctx *ctx, const uint8_t *d_in, size_t n, uint32_t *d_sa_out);
int dk_dev_bwt_forward(dk_ctx *ctx, const uint8_t *d_in, size_t n, uint8_t *d_bwt_out, uint32_t *origin);
/* As dk_bwt_inverse.  On DK_E_STREAM parts of d_out[0, n) may already have been written (unlike the packed inverse below, which checks
 * before it writes); nothing outside [0, n) ever is.  The same holds for the d_out of the block decoders that end in this inverse. */
int dk_dev_bwt_inverse(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, uint32_t origin, uint8_t *d_out);
/* d_dist/d_sym/d_rank: device arrays of n entries (d_rank may be NULL); init and m are returned on the host */
int dk_dev_dc_encode(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, uint32_t init[256],
                     uint32_t *d_dist, uint8_t *d_sym, uint8_t *d_rank, size_t *m);
/* whole forward path from a device-resident block to the coded stream in host memory */
int dk_dev_block_encode(dk_ctx *ctx, int model_id, const uint8_t *d_in, size_t n,
                        uint8_t *out, size_t out_cap, size_t *out_len);
/* `count` independent blocks on one GPU, pipelined: the device stages of block i+1 run while up to `host_threads` host threads
 * code the distance streams of earlier blocks (the reference treats every block as self-contained: fresh model and coder per
 * Encoder::new, src/block/dc.rs:30-37,53).  out[i] / out_len[i] are exactly what dk_dev_block_encode gives for block i. */
int dk_dev_batch_encode(dk_ctx *ctx, int model_id, size_t count, const uint8_t *const *d_in, const size_t *n,
                        uint8_t *const *out, const size_t *out_cap, size_t *out_len, int host_threads);
/* The same pipeline fed one block at a time (blocks that arrive from a file): begin starts `host_threads` coding threads;
 * push runs the device stages of one more block on the calling thread -- on return d_in may be reused -- and queues its coding
 * (it waits while every staging slot is busy); *out_len is written when that block's coding ends; finish waits for all coders,
 * frees the batch and returns the first failure.  Between begin and finish the context serves this batch only: every other entry point
 * returns DK_E_ARG, a second begin included.  A failed push leaves the batch open (earlier blocks are still being coded into the
 * caller's `out` / `out_len`): the caller must still call finish before it frees those buffers.  dk_ctx_destroy finishes a batch that
 * was left open, so the coding threads never outlive the staging memory they read -- and with that the dk_batch handle is GONE: after
 * dk_ctx_destroy it must not be passed to dk_batch_finish (or anything else) any more; the result of that implicit finish is dropped. */
typedef struct dk_batch dk_batch;
int dk_batch_begin(dk_ctx *ctx, int model_id, int host_threads, dk_batch **out);
int dk_batch_push(dk_batch *batch, const uint8_t *d_in, size_t n, uint8_t *out, size_t out_cap, size_t *out_len);
int dk_batch_finish(dk_batch *batch);
/* ---- packed forward path: many blocks laid back to back in ONE device buffer, block i = d_in[off_i, off_i + n[i]) with
 * off_i = n[0] + ... + n[i-1].  One segmented suffix sort and one segmented DC pass serve the whole pack: O(rounds) launches, not O(blocks).
 * Per block, every result equals the single-block entry point's (src/saca.rs:368-378 for L / origin, src/block/dc.rs:41-91 for the DC arrays
 * and the coded stream; the reference treats every block as self-contained, src/block/dc.rs:30-37,53).  A block still unresolved after the
 * pack's round limit (long repeats, e.g. two identical halves) is re-run alone through the single-block path (DK_ROUTE_PACKED_GUARD).
 * DK_E_ARG: count == 0, count > DK_PACKED_MAX_BLOCKS (on a decoder context: > its max_blocks), any n[i] == 0 or > DK_PACKED_MAX_BLOCK_BYTES, sum of n > dk_capacity, null pointers. */
#define DK_PACKED_MAX_BLOCKS 65536
#define DK_PACKED_MAX_BLOCK_BYTES (1u << 24)
/* L of block i at d_bwt_out[off_i, off_i + n[i]), origin[i] (host, count entries) as from dk_dev_bwt_forward */
int dk_dev_bwt_forward_packed(dk_ctx *ctx, const uint8_t *d_in, size_t count, const size_t *n, uint8_t *d_bwt_out, uint32_t *origin);
/* saca::Constructor::compute (src/saca.rs:368-378) for every block of a pack, same layout and limits as dk_dev_bwt_forward_packed:
 * block i's suffix array at d_sa_out[off_i, off_i + n[i]), entries LOCAL to the block (0 .. n[i]-1), equal to what dk_dev_suffix_array
 * gives for block i alone.  d_bwt_out (may be NULL): L of block i at d_bwt_out[off_i, ...) and origin[i] (host, count entries) as from
 * dk_dev_bwt_forward_packed, from the same pass.  origin may be NULL exactly when d_bwt_out is (DK_E_ARG otherwise). */
int dk_dev_suffix_array_packed(dk_ctx *ctx, const uint8_t *d_in, size_t count, const size_t *n, uint32_t *d_sa_out,
                               uint8_t *d_bwt_out, uint32_t *origin);
/* the same from host memory (the reference's &[u8] inputs laid back to back): one upload, one pass, one download */
int dk_suffix_array_packed(dk_ctx *ctx, const uint8_t *in, size_t count, const size_t *n, uint32_t *sa_out);
/* ---- longest-common-prefix arrays (nothing in the reference corresponds: src/saca.rs stops at the suffix array) ---------------------------
 * LCP[0] = 0; for i >= 1, LCP[i] = the number of leading bytes the suffixes SA[i-1] and SA[i] share.  No sentinel (the convention of
 * src/saca.rs:105-113), so LCP[i] <= n - max(SA[i-1], SA[i]).  In a pack every block is on its own: a common prefix ends with the block of
 * the shorter suffix, whatever the next block starts with.  Phi algorithm with irreducible positions, on the device.
 * DK_E_ARG as for the suffix-array entries (null pointers, n == 0, n > dk_capacity, the pack checks, a decoder context), and for an entry of
 * d_sa that is >= n (in a pack: >= n[i]) -- then nothing is written to d_lcp_out.  A d_sa whose entries are in range but which is not the
 * suffix array of the text: the values written are unspecified, but the call returns, every value is <= n (n[i]), and nothing outside
 * [0, n) of the text, d_sa and d_lcp_out is touched.  Whether an array IS the suffix array of its text is what dk_dev_sa_check answers.
 * full_ctx: a DK_CTX_FULL context.  (The parameter's name says so; a decoder context gets DK_E_ARG with the entry's name in dk_last_error.) */
/* d_sa: the suffix array of d_in[0, n) (e.g. from dk_dev_suffix_array); d_lcp_out: n entries.  Any alignment of d_in; d_sa and d_lcp_out
 * need the four bytes of their element only. */
int dk_dev_lcp(dk_ctx *full_ctx, const uint8_t *d_in, size_t n, const uint32_t *d_sa, uint32_t *d_lcp_out);
/* dk_dev_suffix_array, then dk_dev_lcp on its result, in one call (the sort's temporaries are released before the LCP pass takes workspace) */
int dk_dev_suffix_array_lcp(dk_ctx *full_ctx, const uint8_t *d_in, size_t n, uint32_t *d_sa_out, uint32_t *d_lcp_out);
/* the same from and to host memory: one upload, two downloads */
int dk_suffix_array_lcp(dk_ctx *full_ctx, const uint8_t *in, size_t n, uint32_t *sa_out, uint32_t *lcp_out);
/* Layout and limits of dk_dev_suffix_array_packed: block i's suffix array (entries local to the block) at d_sa[off_i, off_i + n[i]), its LCP
 * array to d_lcp_out[off_i, off_i + n[i]), equal to what dk_dev_lcp gives for block i alone.  One pass for the whole pack: the launches do
 * not grow with count. */
int dk_dev_lcp_packed(dk_ctx *full_ctx, const uint8_t *d_in, size_t count, const size_t *n, const uint32_t *d_sa, uint32_t *d_lcp_out);
/* dk_dev_suffix_array_packed (without L), then the LCP arrays, in one call.  The pass takes the packed sort's rank array as the inverse suffix
 * array instead of deriving one; blocks that went through the guard are redone from the suffix arrays the guard wrote. */
int dk_dev_suffix_array_packed_lcp(dk_ctx *full_ctx, const uint8_t *d_in, size_t count, const size_t *n, uint32_t *d_sa_out, uint32_t *d_lcp_out);
/* the same from and to host memory (the layout of dk_suffix_array_packed): one upload, one pass, two downloads */
int dk_suffix_array_packed_lcp(dk_ctx *full_ctx, const uint8_t *in, size_t count, const size_t *n, uint32_t *sa_out, uint32_t *lcp_out);
/* ---- what a caller does with a suffix array: verify it, search in it (nothing in the reference corresponds: src/saca.rs stops at the array;
 * libdivsufsort's sufcheck and sa_search are the models).  DESIGN.md section 4.12.  Layout of a pack as in dk_dev_suffix_array_packed: block i's
 * text at d_in[off_i, off_i + n[i]), its suffix array at d_sa[off_i, off_i + n[i]) with entries LOCAL to the block; every block is on its own.
 * Order as everywhere here (src/saca.rs:105-113): no sentinel, a suffix that is a proper prefix of another sorts first.
 * DK_E_ARG as for the suffix-array entries (null pointers, n == 0, n > dk_capacity, the pack checks, a decoder context).
 * full_ctx: a DK_CTX_FULL context (a decoder context gets DK_E_ARG with the entry's name in dk_last_error).
 *
 * The check.  The return code is DK_OK whenever the check ran: "not a suffix array" is an answer (*verdict), not an error.  verdict and where are
 * HOST memory (packed: count entries each).  Three kinds of failure are tested per block in this order, the first that fails decides and the
 * later ones are not evaluated for that block, so the answer is deterministic; where is local to the block, and n (n[i]) with DK_SA_OK.
 * Linear and exact for any input (Burkhardt, Karkkainen 2003): no stretch of text is compared, a^n costs what random bytes cost. */
#define DK_SA_OK 0u
#define DK_SA_BAD_RANGE 1u        /* where = lowest slot whose entry is >= n_i */
#define DK_SA_NOT_PERMUTATION 2u  /* where = lowest text position that no slot names */
#define DK_SA_BAD_ORDER 3u        /* where = lowest slot i >= 1 whose suffix is not greater than the suffix in slot i-1 */
/* is d_sa[0, n) the suffix array of d_in[0, n)?  Any alignment of d_in; d_sa needs the four bytes of its element only. */
int dk_dev_sa_check(dk_ctx *full_ctx, const uint8_t *d_in, size_t n, const uint32_t *d_sa, uint32_t *verdict, uint32_t *where);
/* the same from host memory: text and array are uploaded (9 n bytes of workspace in all) */
int dk_sa_check(dk_ctx *full_ctx, const uint8_t *in, size_t n, const uint32_t *sa, uint32_t *verdict, uint32_t *where);
/* every block of a pack in one pass (the launches do not grow with count): verdict[i] / where[i] = what dk_dev_sa_check gives for block i alone */
int dk_dev_sa_check_packed(dk_ctx *full_ctx, const uint8_t *d_in, size_t count, const size_t *n, const uint32_t *d_sa,
                           uint32_t *verdict /* [count] */, uint32_t *where /* [count] */);
/* The search.  npat patterns lie back to back in d_pat, pattern q of pat_len[q] bytes (pat_len: HOST memory, like n of the packed calls); for a
 * pack pat_block[q] (HOST) names the block pattern q is searched in.  With "suffix <m P" meaning: the suffix cut to its first m = pat_len[q]
 * bytes is smaller than P as byte strings, a proper prefix being smaller --
 *   d_lo[q] = number of slots of the block whose suffix is <m P,   d_hi[q] = number of slots whose suffix is <=m P   (device, npat entries each),
 * both local to the block, so SA[lo, hi) are exactly the occurrences of P.  A pattern that does not occur gives lo == hi = its insertion slot;
 * m == 0 gives [0, n_i); m > n_i is an ordinary pattern that does not occur.  npat == 0 is DK_OK and writes nothing.
 * DK_E_ARG also for pat_block[q] >= count, more than 2^32 - 1 pattern bytes in all, and, in the host form, patterns plus offsets that do not
 * fit the workspace beside the block.  Workspace: 8 bytes per pattern.
 * The suffix array is TRUSTED, not verified (dk_dev_sa_check does that).  For any array: an entry >= n_i is treated as the empty suffix and the
 * text is not read at it, every compare stops at min(m, n_i - SA[slot]); the results are then unspecified, but lo <= hi <= n_i, and nothing
 * outside the text, the array, the patterns and the two results is touched. */
int dk_dev_sa_search(dk_ctx *full_ctx, const uint8_t *d_in, size_t n, const uint32_t *d_sa,
                     const uint8_t *d_pat, size_t npat, const size_t *pat_len, uint32_t *d_lo, uint32_t *d_hi);
/* the same from and to host memory: text, array and patterns are uploaded, lo and hi downloaded */
int dk_sa_search(dk_ctx *full_ctx, const uint8_t *in, size_t n, const uint32_t *sa,
                 const uint8_t *pat, size_t npat, const size_t *pat_len, uint32_t *lo, uint32_t *hi);
/* patterns searched in the blocks of a pack, one launch for all of them */
int dk_dev_sa_search_packed(dk_ctx *full_ctx, const uint8_t *d_in, size_t count, const size_t *n, const uint32_t *d_sa,
                            const uint8_t *d_pat, size_t npat, const size_t *pat_len, const uint32_t *pat_block,
                            uint32_t *d_lo, uint32_t *d_hi);
/* ---- matching statistics and super-maximal exact matches of query texts against a block (csrc/sa_query.hip) ----
 * Which stretches of a query does the block already hold, and how long is each?  Text, suffix array and packs as for the search above; nq
 * queries lie back to back in d_query, query j of query_len[j] bytes (HOST memory, as pat_len), for a pack matched against block query_block[j]
 * (HOST).  Q = the sum of the lengths; a POSITION g in [0, Q) lies in query j at offset i, and its window is the m_g = min(max_len,
 * query_len[j] - i) bytes from it on: a window never runs into the next query.
 *   d_len[g] = the largest l <= m_g such that d_query[g, g + l) occurs in the block;
 *   d_lo[g], d_hi[g] = what dk_dev_sa_search gives for that pattern of l bytes, local to the block (l == 0: [0, n_i)), so SA[lo, hi) are the
 *   occurrences of the longest match and hi > lo.  d_lo and d_hi may BOTH be null: only the lengths are written.  Q entries each.
 * A position g is reported as a super-maximal match (SMEM) when, with capped(g) meaning len[g] == max_len,
 *   len[g] >= max(min_len, 1);   i == 0 or len[g - 1] <= len[g] (the match one byte earlier does not contain this one);   and not (i > 0 and
 *   capped(g - 1) and capped(g)): a copy longer than max_len is reported once, at its first position, with len = max_len.
 * Without a cap these are exactly the matches of a query that no other match of the same query contains.  The record's `at` is the position g,
 * an offset into d_query; the caller maps it to (query, offset) through the lengths.  The first min(*total, max_hits) records are written in
 * rising order of `at` (device records 16-byte aligned); *total (HOST, 64 bits) is complete when the list is cut; max_hits == 0 counts only
 * and d_hits may be null.  Placement is by an exclusive scan of the flags: no atomics, the same bytes in every run, and nothing behind the
 * last record written is touched.
 * DK_E_ARG as for the search (nulls, n == 0, the pack checks, query_block[j] >= count, more than 2^32 - 1 query bytes, a decoder context),
 * and for max_len == 0, exactly one of d_lo / d_hi null, records off their alignment, and what does not fit the workspace: the device forms of
 * match take 8 bytes per query, those of smems 16 bytes per query byte more; the host forms upload text, array and queries beside that.
 * max_len above 2^32 - 1 counts as 2^32 - 1.  nq == 0 or Q == 0 is DK_OK, writes nothing and gives *total = 0; empty queries among others
 * are allowed.  The suffix array is TRUSTED, as in the search.  For any array: an entry >= n_i is the empty suffix and the text is not read
 * at it, every compare stops at min(m_g, n_i - SA[slot]), every step shrinks its range; the results are then unspecified, but len[g] <= m_g
 * and lo <= hi <= n_i, and nothing outside the text, the array, the queries and the outputs is touched. */
typedef struct dk_sa_smem { uint32_t at, len, lo, hi; } dk_sa_smem; /* 16 bytes */
int dk_dev_sa_match(dk_ctx *full_ctx, const uint8_t *d_in, size_t n, const uint32_t *d_sa, const uint8_t *d_query, size_t nq,
                    const size_t *query_len, size_t max_len, uint32_t *d_len, uint32_t *d_lo, uint32_t *d_hi);
int dk_dev_sa_match_packed(dk_ctx *full_ctx, const uint8_t *d_in, size_t count, const size_t *n, const uint32_t *d_sa, const uint8_t *d_query,
                           size_t nq, const size_t *query_len, const uint32_t *query_block, size_t max_len,
                           uint32_t *d_len, uint32_t *d_lo, uint32_t *d_hi);
/* the same from and to host memory: text, array and queries are uploaded, the statistics downloaded */
int dk_sa_match(dk_ctx *full_ctx, const uint8_t *in, size_t n, const uint32_t *sa, const uint8_t *query, size_t nq, const size_t *query_len,
                size_t max_len, uint32_t *len, uint32_t *lo, uint32_t *hi);
int dk_dev_sa_smems(dk_ctx *full_ctx, const uint8_t *d_in, size_t n, const uint32_t *d_sa, const uint8_t *d_query, size_t nq,
                    const size_t *query_len, size_t min_len, size_t max_len, size_t max_hits, dk_sa_smem *d_hits, uint64_t *total);
int dk_dev_sa_smems_packed(dk_ctx *full_ctx, const uint8_t *d_in, size_t count, const size_t *n, const uint32_t *d_sa, const uint8_t *d_query,
                           size_t nq, const size_t *query_len, const uint32_t *query_block, size_t min_len, size_t max_len, size_t max_hits,
                           dk_sa_smem *d_hits, uint64_t *total);
int dk_sa_smems(dk_ctx *full_ctx, const uint8_t *in, size_t n, const uint32_t *sa, const uint8_t *query, size_t nq, const size_t *query_len,
                size_t min_len, size_t max_len, size_t max_hits, dk_sa_smem *hits, uint64_t *total);
/* ---- FM-index: count patterns in a BWT, without the text and without a suffix array (csrc/fm_index.hip) ----
 * Backward search on L itself.  The index is an opaque DEVICE buffer of dk_fm_index_bytes(total, count) bytes that the caller supplies (4-byte
 * aligned): checkpointed symbol counts of the pack every 1024 positions and 1040 bytes per block, about `total` bytes in all; with L itself
 * about 2 n bytes stay resident, against the 5 n of text and suffix array that dk_dev_sa_search needs.  dk_fm_index_bytes needs no GPU and
 * returns 0 for what the pack checks refuse (total == 0 or > 2^31 - 2, count == 0 or > DK_PACKED_MAX_BLOCKS, count > total).
 * (d_bwt, origin) are what dk_dev_bwt_forward / dk_dev_bwt_forward_packed / dk_stream_decode give; d_bwt, any alignment, must stay as it was
 * when the index was built.  dk_dev_fm_count* give, for the same patterns in the same layout (pat_len / pat_block in HOST memory), exactly
 * the d_lo / d_hi of dk_dev_sa_search*, insertion slots of absent patterns included; hi - lo = the number of occurrences.  Same error cases;
 * also DK_E_ARG for origin >= n and an index that is not 4-byte aligned.  The recurrence is defined for ANY bytes L and any origin < n.
 * any_ctx: a context of EITHER purpose, as the parameter's name says (full_ctx above: DK_CTX_FULL only): decoder contexts serve every entry
 * of this section; their own max_blocks limits a pack.  Workspace: the build takes at most
 * 256 KiB + 8 bytes per block, the count 8 bytes per pattern + 4 per block.
 * The index is TRUSTED.  For any bytes in it, in L and in the patterns the geometry is the caller's, every position is clamped to its block
 * before use: results are then unspecified but <= n_i, and nothing outside L, the index, the patterns and the two results is touched. */
size_t dk_fm_index_bytes(size_t total, size_t count);
int dk_dev_fm_build(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t n, uint32_t origin, void *d_index);
int dk_dev_fm_build_packed(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const uint32_t *origin /* host */, void *d_index);
int dk_dev_fm_count(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t n, const void *d_index,
                    const uint8_t *d_pat, size_t npat, const size_t *pat_len, uint32_t *d_lo, uint32_t *d_hi);
int dk_dev_fm_count_packed(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const void *d_index,
                           const uint8_t *d_pat, size_t npat, const size_t *pat_len, const uint32_t *pat_block, uint32_t *d_lo, uint32_t *d_hi);
/* from and to host memory: L and the patterns are uploaded, the index built, lo and hi downloaded.  DK_E_ARG when L, the index, the patterns,
 * their offsets and the results (about 2 n + the patterns + 12 bytes per pattern) do not fit the workspace. */
int dk_fm_count(dk_ctx *any_ctx, const uint8_t *bwt, size_t n, uint32_t origin,
                const uint8_t *pat, size_t npat, const size_t *pat_len, uint32_t *lo, uint32_t *hi);
/* ---- FM-index: locate.  Where the occurrences are, from a sampled suffix array (csrc/bwt.hip, csrc/fm_index.hip) ----
 * A second opaque DEVICE buffer of the caller's beside the index: dk_fm_locate_bytes(total, count, step) bytes, 4-byte aligned.  It marks the
 * slots whose suffix starts at a multiple of `step` (positions local to the block; position 0 always) and keeps position / step of each: about
 * total / 8 + 4 total / step bytes, 0.26 n at step 32.  dk_fm_locate_bytes needs no GPU; 0 for what dk_fm_index_bytes refuses and for a step
 * that is no power of two in [1, 4096].
 * dk_dev_fm_locate_build* need (L, origin) only -- neither the index nor a suffix array: they run the inverse BWT's successor table, splitter
 * walk and jumps, and two more walks in place of the one that writes the text.  DK_E_STREAM, exactly where dk_dev_bwt_inverse* gives it, when
 * (L, origin) describe no text (in a pack the message names the lowest such block); d_loc is then unspecified.  DK_E_ARG as for
 * dk_dev_fm_build*, for a bad step and a d_loc that is not 4-byte aligned; a pack obeys DK_PACKED_MAX_BLOCK_BYTES and the context's max_blocks.
 * Workspace: the packed inverse's without its walk records, which every context that can invert the block or pack holds.
 * dk_dev_fm_locate*: d_lo / d_hi (device, npat words each) as dk_dev_fm_count* wrote them, `step` the one of the build.  Row q of d_pos
 * (device, npat x max_hits words): d_pos[q max_hits + j] = SA_b[lo[q] + j] for j < min(hi[q] - lo[q], max_hits), in suffix-array order,
 * DK_FM_NO_HIT behind them: no scan, no readback.  The empty pattern's range [0, n) with max_hits = n gives the whole suffix array.
 * DK_E_ARG for max_hits == 0, npat x max_hits > 2^31, pat_block[q] >= count (pat_block in HOST memory), null or misaligned pointers.
 * Both structures are TRUSTED, and contained as the count is: lo and hi are clamped to [0, n_b] (hi < lo: no hits), every slot to [0, n_b),
 * the sample's index to the samples, and at most min(step, n_b) steps are taken; for any bytes in L, the index, d_loc, d_lo and d_hi every
 * value written is < n_b or DK_FM_NO_HIT, and nothing outside those buffers and d_pos is touched. */
#define DK_FM_NO_HIT 0xFFFFFFFFu
size_t dk_fm_locate_bytes(size_t total, size_t count, uint32_t step);
int dk_dev_fm_locate_build(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t n, uint32_t origin, uint32_t step, void *d_loc);
int dk_dev_fm_locate_build_packed(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const uint32_t *origin /* host */,
                                  uint32_t step, void *d_loc);
int dk_dev_fm_locate(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t n, const void *d_index, const void *d_loc, uint32_t step,
                     const uint32_t *d_lo, const uint32_t *d_hi, size_t npat, size_t max_hits, uint32_t *d_pos);
int dk_dev_fm_locate_packed(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const void *d_index, const void *d_loc,
                            uint32_t step, const uint32_t *d_lo, const uint32_t *d_hi, size_t npat, const uint32_t *pat_block /* host */,
                            size_t max_hits, uint32_t *d_pos);
/* from and to host memory: upload, both builds, count, locate, download of lo, hi (npat words each) and pos (npat x max_hits).  DK_E_ARG
 * when L, the two structures, the batch, its results and the locate build's workspace do not fit the context's workspace. */
int dk_fm_locate(dk_ctx *any_ctx, const uint8_t *bwt, size_t n, uint32_t origin, uint32_t step, const uint8_t *pat, size_t npat,
                 const size_t *pat_len, size_t max_hits, uint32_t *lo, uint32_t *hi, uint32_t *pos);
/* ---- FM-index: extract.  What the text says at given positions, from L, the index and sampled inverse-suffix-array entries (csrc/bwt.hip,
 * csrc/fm_index.hip) ----
 * A third opaque DEVICE buffer of the caller's: dk_fm_extract_bytes(total, count, step) bytes, 4-byte aligned.  It keeps, for every block, the
 * slot of the suffix that starts at each multiple of `step` (the block's ANCHORS; positions local to the block): 4 (total / step + count) + 256
 * bytes, 0.125 n at step 32.  dk_fm_extract_bytes needs no GPU; 0 for what dk_fm_index_bytes refuses and for a step that is no power of two in
 * [1, 4096].
 * dk_dev_fm_extract_build* need (L, origin) only: the front part of dk_dev_fm_locate_build* -- the inverse BWT's successor table, splitter walk
 * and jumps -- and one more walk that stores the anchors.  DK_E_STREAM, DK_E_ARG and the workspace exactly as for dk_dev_fm_locate_build*
 * (4 bytes per block more).
 * dk_dev_fm_extract*: d_pos / d_len (device, nrange words each; d_len may be null: every range is max_len long) are start positions local to
 * the range's block and lengths; a row of dk_dev_fm_locate's d_pos can be passed as it is.  Row q of d_out (device, nrange x max_len BYTES, any
 * alignment) = T_b[pos[q] + j] for j < got[q] = min(len[q], max_len, n_b - pos[q]), zero bytes behind them; got[q] = 0 for pos[q] >= n_b,
 * DK_FM_NO_HIT included.  `step` is the one of the build.  One range (0, n) with max_len = n gives the whole text.  nrange == 0: DK_OK, nothing
 * written.  DK_E_ARG for max_len == 0, nrange x max_len > 2^31, range_block[q] >= count (range_block in HOST memory), null or misaligned word
 * pointers, a bad step.  Workspace: 8 bytes; in a pack 8 bytes per block and 4 per range.
 * Both structures are TRUSTED, and contained as count and locate are: every slot is clamped to [0, n_b), every anchor index to the block's
 * anchors, at most min(step, n_b) steps are taken per (range, chunk of `step` positions), stores go to row q's max_len bytes only; for any
 * bytes in L, the index, d_ext, d_pos and d_len every byte written is a byte of block b's L or zero, and nothing outside those buffers and
 * d_out is touched. */
size_t dk_fm_extract_bytes(size_t total, size_t count, uint32_t step);
int dk_dev_fm_extract_build(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t n, uint32_t origin, uint32_t step, void *d_ext);
int dk_dev_fm_extract_build_packed(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const uint32_t *origin /* host */,
                                   uint32_t step, void *d_ext);
int dk_dev_fm_extract(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t n, const void *d_index, const void *d_ext, uint32_t step,
                      const uint32_t *d_pos, const uint32_t *d_len, size_t nrange, size_t max_len, uint8_t *d_out);
int dk_dev_fm_extract_packed(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const void *d_index, const void *d_ext,
                             uint32_t step, const uint32_t *d_pos, const uint32_t *d_len, size_t nrange, const uint32_t *range_block /* host */,
                             size_t max_len, uint8_t *d_out);
/* from and to host memory: upload, both builds, extract, download of the nrange x max_len rows (len may be null).  DK_E_ARG when L, the two
 * structures, the ranges, the rows and the larger build workspace do not fit the context's workspace. */
int dk_fm_extract(dk_ctx *any_ctx, const uint8_t *bwt, size_t n, uint32_t origin, uint32_t step, const uint32_t *pos, const uint32_t *len,
                  size_t nrange, size_t max_len, uint8_t *out);
/* ---- FM-index: find.  Every pattern in every block, as one compact list of hits (csrc/fm_index.hip) ----
 * The query of an archive search: the patterns are given once (layout of dk_dev_fm_count, no pat_block) and the grid (pattern q, block b) is
 * walked on the device.  With [lo, hi) = what dk_dev_fm_count_packed gives for q in b:
 *   d_occ[q * count + b] = hi - lo (0 where an index that is none gives hi < lo); d_occ (device, npat x count words) may be null
 *   *total (HOST, 64 bits) = the sum of all occ
 *   the hits, in ascending order of (q, b, j), j < occ, are the records {q, b, SA_b[lo + j], lo + j}: `position` is exactly what
 *   dk_dev_fm_locate_packed writes for that slot (DK_FM_NO_HIT included), and the order inside a pair is its order
 *   d_hits (device, 16-byte aligned) receives the first min(*total, max_hits) records; nothing behind them is written.
 * max_hits == 0 is allowed: d_hits and d_loc may then be null, and only d_occ and *total come back.  The empty pattern counts every position.
 * The order is fixed by an exclusive scan of occ over the pairs; no global atomics, so two calls give the same bytes.
 * DK_E_ARG for what dk_dev_fm_count* and dk_dev_fm_locate* refuse (null or misaligned structures, a bad step, a bad pack), for npat x count >
 * DK_FM_FIND_MAX_PAIRS, max_hits > 2^31, a d_hits that is not 16-byte aligned, a null `total`, and for a workspace that cannot hold the
 * pattern offsets, 4 bytes per block and 16 bytes per pair.  DK_FM_FIND_MAX_PAIRS is a reasoned bound (256 MiB of workspace), not a measured one.
 * Contained as count and locate are: lo and hi are clamped to [0, n_b], every slot to [0, n_b), the pair a hit belongs to to the pairs, and
 * at most min(step, n_b) steps are taken per hit; for any bytes in L, the index and d_loc every record written has pattern < npat, block <
 * count, slot < n_b and position < n_b or DK_FM_NO_HIT, and nothing outside the named buffers is touched. */
typedef struct dk_fm_hit { uint32_t pattern, block, position, slot; } dk_fm_hit; /* 16 bytes */
#define DK_FM_FIND_MAX_PAIRS (1u << 24)
int dk_dev_fm_find(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t n, const void *d_index, const void *d_loc, uint32_t step, const uint8_t *d_pat,
                   size_t npat, const size_t *pat_len /* host */, size_t max_hits, dk_fm_hit *d_hits, uint32_t *d_occ /* may be NULL */,
                   uint64_t *total /* host */);
int dk_dev_fm_find_packed(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const void *d_index, const void *d_loc,
                          uint32_t step, const uint8_t *d_pat, size_t npat, const size_t *pat_len /* host */, size_t max_hits, dk_fm_hit *d_hits,
                          uint32_t *d_occ /* may be NULL */, uint64_t *total /* host */);
/* from and to host memory: upload, the builds (the locate structure only when max_hits > 0), find, download of min(*total, max_hits) records
 * and of occ (npat words; may be null).  DK_E_ARG when L, the structures, the batch and the records do not fit the context's workspace. */
int dk_fm_find(dk_ctx *any_ctx, const uint8_t *bwt, size_t n, uint32_t origin, uint32_t step, const uint8_t *pat, size_t npat,
               const size_t *pat_len, size_t max_hits, dk_fm_hit *hits, uint32_t *occ, uint64_t *total);
/* ---- FM-index: seams.  The matches that straddle block borders (csrc/fm_index.hip) ----
 * dk_dev_fm_find* search every block on its own.  Here a pack's blocks 0 .. count - 1, in pack order and preceded by prev_len >= 0 carried
 * bytes d_prev (device; piece -1), are the consecutive PIECES of one text.  A SEAM HIT of pattern q (m bytes) is an occurrence in that
 * concatenation whose first and last byte lie in different pieces.  It belongs to the block b that holds its LAST byte, and `back` in
 * [1, m - 1] is the number of its bytes in front of block b's first byte; they may span several tiny blocks and reach into prev.  Patterns of
 * 0 and 1 bytes have no seam hits, and an occurrence wholly inside one piece (prev included) is none: find reports those.  For any cutting
 * of a file into blocks and packs, the hits of find and the seam hits with prev = the last bytes in front of the pack are together exactly
 * the occurrences in the file, each once.
 *   d_occ[q * count + b] (device, may be null) = seam hits of q that belong to b;  *total (HOST, 64 bits) = their sum
 *   d_hits (device, 16-byte aligned) receives the first min(*total, max_hits) records {q, b, back, 0} in the order (q, b, back descending),
 *   the file order of the starts inside a pair; nothing behind them is written.  max_hits == 0: d_hits may be null, counts only.
 * The order comes from an exclusive scan of occ over the pairs; no global atomics, so two calls give the same bytes.
 * dk_dev_fm_seams is the single-block form: its only border is the one against prev.  There is NO host-memory form: a single block has no
 * inner border, and find has no packed host form either.  Contexts of either purpose serve both.  `step` is the extract structure's.
 * DK_E_ARG for what dk_dev_fm_find* and dk_dev_fm_extract* refuse (null or misaligned structures, a bad step, a bad pack), a pattern longer
 * than DK_FM_SEAM_MAX_PATTERN, prev_len >= DK_FM_SEAM_MAX_PATTERN (only the last longest - 1 carried bytes can matter), prev_len > 0 with a
 * null d_prev, npat x count > DK_FM_FIND_MAX_PAIRS, max_hits > 2^31, a d_hits that is not 16-byte aligned, a null `total`, and for a
 * workspace that cannot hold the edge strip (at most prev_len + min(total, 2 (longest - 1) count) bytes), 52 bytes per block, the pattern
 * offsets and 16 bytes per pair.  dk_workspace_bytes does not grow for it.  DK_FM_SEAM_MAX_PATTERN is a reasoned bound, not a measured one:
 * the window at a border stays a few KiB and the quadratic worst case (a periodic pattern on a periodic text) stays bounded.
 * Both structures are TRUSTED and contained as find and extract are: the strip's layout comes from the sizes, never from the structures;
 * every strip index is clamped to the strip; for any bytes in L, the index, d_ext and d_prev every record written has pattern < npat,
 * block < count and 1 <= back < m, and nothing outside the named buffers is touched. */
typedef struct dk_fm_seam_hit { uint32_t pattern, block, back, reserved /* 0 */; } dk_fm_seam_hit; /* 16 bytes */
#define DK_FM_SEAM_MAX_PATTERN 4096u
int dk_dev_fm_seams(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t n, const void *d_index, const void *d_ext, uint32_t step,
                    const uint8_t *d_prev, size_t prev_len, const uint8_t *d_pat, size_t npat, const size_t *pat_len /* host */, size_t max_hits,
                    dk_fm_seam_hit *d_hits, uint32_t *d_occ /* may be NULL */, uint64_t *total /* host */);
int dk_dev_fm_seams_packed(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const void *d_index, const void *d_ext,
                           uint32_t step, const uint8_t *d_prev, size_t prev_len, const uint8_t *d_pat, size_t npat,
                           const size_t *pat_len /* host */, size_t max_hits, dk_fm_seam_hit *d_hits, uint32_t *d_occ /* may be NULL */,
                           uint64_t *total /* host */);
/* ---- FM-index: near.  Byte classes and a budget of mismatches (csrc/fm_index.hip) ----
 * dk_dev_fm_find* with patterns that are sequences of BYTE CLASSES and with up to k positions missed.  Position j of pattern q is a set of
 * byte values given as 32 bytes: bit c & 7 of byte c >> 3 is set when byte value c matches (one bit: an exact byte; two: an ASCII letter under
 * ignore-case; all 256: a wildcard; none: legal, never matches for free).  The classes of all patterns lie back to back in d_cls (device,
 * 32 x the sum of pat_len bytes, any alignment); pat_len in HOST memory, as for find.
 * The COST of a string w of m bytes against pattern q (m positions) is the number of positions i with w[i] outside cls_q[i]: the Hamming
 * distance, no insertions or deletions.  The NEAR HITS of q in block b are the positions p in [0, n_b - m] whose text T_b[p, p + m) has cost
 * <= k, each once, with its cost; a match lies wholly inside its block.  The empty pattern has n_b hits of cost 0.  With k = 0 and one-bit
 * classes the set of (pattern, block, position) is find's.
 * THE SEARCH TREE fixes the order and the node limit.  A node is (j, w): 0 <= j <= m, w a string of m - j bytes that occurs wholly inside
 * block b with cost <= k against cls_q[j .. m).  The root is (m, ""), the children of (j, w) are the nodes (j - 1, c w) in ascending order
 * of c, the leaves are the nodes with j = 0.  The records stand in ascending order of (pattern, block, leaf in preorder, suffix-array slot
 * inside the leaf's range) -- the leaves in the order of the matched strings compared from their LAST byte to their first.  The order comes
 * from an exclusive scan of the pairs' counts; no global atomics, two calls give the same bytes.
 * Each pair visits at most node_limit nodes, the first min(node_limit, N) of its N in preorder, the root being the first; its hits are the
 * leaves among them, a prefix of its whole list, and the pair is CUT when N > node_limit.  node_limit = 0: DK_FM_NEAR_NODE_LIMIT.
 *   d_occ[q * count + b] (device, may be null) = the hits found for the pair, a lower bound where the pair was cut
 *   *total (HOST, 64 bits) = their sum; *cut (HOST, may be null) = the number of cut pairs
 *   d_hits (device, 16-byte aligned) receives the first min(*total, max_hits) records; nothing behind them is written.  `position` is what
 *   dk_dev_fm_locate_packed gives for the slot, DK_FM_NO_HIT included.  max_hits == 0 counts only: d_hits and d_loc may be null.
 * Contexts of either purpose serve both entries.  There is NO host-memory form and NO C++ mirror (include/dark.hpp) of near.
 * DK_E_ARG for what dk_dev_fm_find* refuses, a pattern longer than DK_FM_NEAR_MAX_PATTERN, k > DK_FM_NEAR_MAX_K, a null d_cls with patterns
 * that are not all empty, npat x count > DK_FM_FIND_MAX_PAIRS, max_hits > 2^31, a misaligned d_hits, a null `total`, and a workspace that
 * cannot hold the pattern offsets, 4 bytes per block and 16 bytes per pair.  dk_workspace_bytes does not grow for it.
 * The three constants are REASONED, NOT MEASURED: 128 positions keep four waves' stacks at about 23 KB of LDS per workgroup, 3 is where
 * Hamming search on an index is still commonly used, 2^20 nodes is a guess at "well under a second for one wave".
 * Contained as find is: the geometry is the caller's, every slot is clamped, the stack's depth is bounded by m, the nodes by the limit and
 * the children tried per node by 256; for any bytes in L, the index, d_loc and d_cls the call returns, every record has pattern < npat,
 * block < count, cost <= k and position < n_b or DK_FM_NO_HIT, and nothing outside the named buffers is touched. */
typedef struct dk_fm_near_hit { uint32_t pattern, block, position, cost; } dk_fm_near_hit; /* 16 bytes */
#define DK_FM_NEAR_MAX_PATTERN 128u
#define DK_FM_NEAR_MAX_K 3u
#define DK_FM_NEAR_NODE_LIMIT (1u << 20)
int dk_dev_fm_near(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t n, const void *d_index, const void *d_loc, uint32_t step,
                   const uint8_t *d_cls, size_t npat, const size_t *pat_len /* host */, uint32_t k, uint32_t node_limit, size_t max_hits,
                   dk_fm_near_hit *d_hits, uint32_t *d_occ /* may be NULL */, uint64_t *total /* host */, uint64_t *cut /* host, may be NULL */);
int dk_dev_fm_near_packed(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const void *d_index, const void *d_loc,
                          uint32_t step, const uint8_t *d_cls, size_t npat, const size_t *pat_len /* host */, uint32_t k, uint32_t node_limit,
                          size_t max_hits, dk_fm_near_hit *d_hits, uint32_t *d_occ /* may be NULL */, uint64_t *total /* host */,
                          uint64_t *cut /* host, may be NULL */);
/* for the tests: d_out[q] = occurrences of d_sym[q] in d_bwt[0, min(d_pos[q], total)), computed by the count kernel's rank (all device memory) */
int dk_dbg_dev_fm_rank(dk_ctx *any_ctx, const uint8_t *d_bwt, size_t total, const void *d_index,
                       const uint32_t *d_pos, const uint8_t *d_sym, size_t nq, uint32_t *d_out);
/* DC arrays of a packed L: block i's entries at [off_i, off_i + m[i]) of d_dist / d_sym / d_rank (device, sum of n entries each; d_rank may
 * be NULL), init (host, count x 256: block i's table at init[256 i]) and m (host, count) as from dk_dev_dc_encode */
int dk_dev_dc_encode_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, uint32_t *init, uint32_t *d_dist, uint8_t *d_sym,
                            uint8_t *d_rank, size_t *m);
/* every block of the pack queued as its own coding job of an open batch (out[i] / out_len[i] as from dk_dev_block_encode); the pack's
 * distance stream takes one staging slot, released when its last block is coded.  flags (may be NULL): flags[i] = what dk_last_block_flags
 * gives after block i alone.  On return d_in may be reused. */
int dk_batch_push_packed(dk_batch *batch, const uint8_t *d_in, size_t count, const size_t *n, uint8_t *const *out, const size_t *out_cap,
                         size_t *out_len, unsigned *flags);
/* dk_batch_begin + dk_batch_push_packed + dk_batch_finish */
int dk_dev_packed_encode(dk_ctx *ctx, int model_id, const uint8_t *d_in, size_t count, const size_t *n, uint8_t *const *out, const size_t *out_cap,
                         size_t *out_len, unsigned *flags, int host_threads);
/* Packed inverse, the same layout and limits: ONE segmented inverse BWT for every block of the pack (launches follow the largest block, not
 * count).  Inverse of dk_dev_bwt_forward_packed: block i's text at d_out[off_i, off_i + n[i]) from L at d_bwt[off_i, ...) and origin[i] (host).
 * DK_E_ARG also for origin[i] >= n[i].  DK_E_STREAM when a block's (L, origin) is not a single text cycle: dk_last_error names the block,
 * nothing is written to d_out, and the context stays usable. */
int dk_dev_bwt_inverse_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const uint32_t *origin, uint8_t *d_out);
/* Inverse of dk_dev_packed_encode: up to host_threads host threads decode the streams into one pinned pack-sized slot, then ONE upload and ONE
 * packed inverse; d_out holds the blocks back to back.  DK_E_MODEL for rawdc and unknown models; DK_E_STREAM naming the block for a stream that
 * does not decode or a decoded origin outside its block.  One-symbol blocks are returned whole, as by dk_dev_batch_decode. */
int dk_dev_packed_decode(dk_ctx *ctx, int model_id, size_t count, const uint8_t *const *in, const size_t *in_len, const size_t *n,
                         uint8_t *d_out, int host_threads);
/* inverse of dk_dev_batch_encode: host threads decode the streams while the GPU inverts the BWTs that are ready */
int dk_dev_batch_decode(dk_ctx *ctx, int model_id, size_t count, const uint8_t *const *in, const size_t *in_len, const size_t *n,
                        uint8_t *const *d_out, int host_threads);
/* whole inverse path from a coded stream in host memory to a device-resident block */
int dk_dev_block_decode(dk_ctx *ctx, int model_id, const uint8_t *in, size_t in_len, size_t n, uint8_t *d_out);

/* ---- several GPUs in one call ------------------------------------------------------------------------------------------------------
 * Blocks are independent (fresh model and coder per block, src/block/dc.rs:30-37,53): block i goes to GPU devices[i mod ndev].  Inside
 * the call every listed device gets one host thread with its own dk_ctx ("one host thread + one context per GPU",
 * no inter-GPU traffic); each runs the pipelined batch path on its blocks with host_threads_per_gpu coding threads.  `devices` may name
 * a GPU twice (two contexts on one GPU).  in / out are host pointers; out[i] / out_len[i] are exactly what dk_block_encode gives for
 * block i.  err (may be NULL) receives the text of the first failure. */
int dk_multi_block_encode(const int *devices, int ndev, int model_id, size_t count, const uint8_t *const *in, const size_t *n,
                          uint8_t *const *out, const size_t *out_cap, size_t *out_len, int host_threads_per_gpu, char *err, size_t err_cap);
int dk_multi_block_decode(const int *devices, int ndev, int model_id, size_t count, const uint8_t *const *in, const size_t *in_len,
                          const size_t *n, uint8_t *const *out, int host_threads_per_gpu, char *err, size_t err_cap);

/* ---- model / coder level (host; what src/model/mod.rs:59-76 and src/entropy/ari.rs:76-107 exercise) ----------- */
/* model.reset(); for k: model.encode(dist[k], Context{symbol: sym[k]}, eh); eh.finish()   (src/model/mod.rs:59-66) */
int dk_model_encode(int model_id, const uint32_t *dist, const uint8_t *sym, size_t m,
                    uint8_t *out, size_t out_cap, size_t *out_len);
/* model.reset(); for k: dist[k] = model.decode(Context{symbol: sym[k]}, dh)              (src/model/mod.rs:67-75) */
int dk_model_decode(int model_id, const uint8_t *in, size_t in_len, const uint8_t *sym, size_t m, uint32_t *dist);
/* entropy::Encoder over entropy::ari::Range (src/entropy/mod.rs:11-41, src/entropy/ari.rs:8-74):
 * bits[k] in {0,1}; flat[k] = apm::Bit::to_flat() = 12-bit probability of a zero */
int dk_bitcoder_encode(const uint8_t *bits, const uint16_t *flat, size_t nbits,
                       uint8_t *out, size_t out_cap, size_t *out_len);
int dk_bitcoder_decode(const uint8_t *in, size_t in_len, const uint16_t *flat, size_t nbits, uint8_t *bits);

/* Host entropy stage on its own (what the GPU stages feed): src/block/dc.rs:53-90 from (init, dist[m], sym[m], origin) to the
 * coded stream, and src/block/dc.rs:121-151 back to (BWT, origin).  rank/run_end (Context.last_rank and the position of each
 * entry) are only read by DK_MODEL_RAWDC and may be NULL otherwise.  *single_symbol = 1 flags a one-symbol block, for which the
 * reference mis-reads `origin` (DESIGN.md "Reference quirks"). */
int dk_stream_encode(int model_id, size_t n, const uint32_t init[256], const uint32_t *dist, const uint8_t *sym,
                     const uint8_t *rank, const uint32_t *run_end, size_t m, uint32_t origin,
                     uint8_t *out, size_t out_cap, size_t *out_len);
int dk_stream_decode(int model_id, const uint8_t *in, size_t in_len, size_t n, uint8_t *bwt_out, uint32_t *origin,
                     int *single_symbol, size_t *consumed /* may be NULL: bytes of `in` read = the length the encoder wrote */);

/* Host half of block::raw on its own (what the GPU BWT feeds / is fed by): src/block/raw.rs:45-58 from (L, origin) to the coded stream and
 * src/block/raw.rs:85-97 back.  raw_model must be a coding model (DK_RAWMODEL_BBB). */
int dk_raw_stream_encode(int raw_model, const uint8_t *bwt, size_t n, uint32_t origin, uint8_t *out, size_t out_cap, size_t *out_len);
int dk_raw_stream_decode(int raw_model, const uint8_t *in, size_t in_len, size_t n, uint8_t *bwt_out, uint32_t *origin, size_t *consumed);

/* ---- measurement ------------------------------------------------------------------------------------------ */
#define DK_NUM_KERNEL_SLOTS 32
typedef struct dk_stats {
    /* wall-clock stage times of the last block call on this context, milliseconds */
    double ms_h2d, ms_sa, ms_bwt, ms_dc, ms_d2h, ms_entropy, ms_ibwt, ms_total;
    /* ms_d2h of a large single block (>= 2^21 distances, dk_block_encode / dk_dev_block_encode): the distance stream leaves the GPU in pieces
     * while the host coder already runs, so ms_d2h = the time to enqueue the copies + the time the call waits for the stream after coding
     * (normally microseconds: the transfer hides behind the coder); the coder's own waits at the frontier are part of ms_entropy. */
    uint32_t rounds;          /* prefix-doubling rounds executed by the last suffix sort */
    uint32_t sort_passes;     /* radix passes executed by the last suffix sort */
    uint64_t sorted_elements; /* sum over passes of elements moved */
    uint64_t dc_runs;         /* m of the last dc encode */
    uint32_t entropy_threads; /* host threads the last range-coder pass used: 1, 2 (models | coder), 4 (exponent model, mantissa model, merger, coder), 5 (the exponent model in two halves) or 6 (five stages and a prepare stage in front of the coder) */
    int32_t entropy_l3_group; /* the last-level-cache group that pass claimed for its threads (lowest cpu number in it); -1: none */
    /* per-kernel HIP-event timings accumulated since dk_stats_reset (only while profiling is enabled) */
    uint32_t kernel_launches[DK_NUM_KERNEL_SLOTS];
    double kernel_ms[DK_NUM_KERNEL_SLOTS];
    double kernel_bytes[DK_NUM_KERNEL_SLOTS]; /* algorithmic bytes summed over launches */
    uint32_t sa_route;        /* DK_ROUTE_* bits: which ways through the suffix sort the last call took (tests assert the route they are named after) */
    int16_t entropy_l3_numa;  /* memory node of that group (-1: none claimed / unknown) ... */
    int16_t gpu_numa;         /* ... and of the context's GPU (/sys/bus/pci/devices/<bdf>/numa_node; -1: unknown): the coder looks for its group there first */
    uint64_t ws_peak_bytes;   /* most the context's device workspace has held at once since dk_ctx_create ... */
    uint64_t ws_size_bytes;   /* ... and its size = dk_workspace_bytes of the context's purpose (full: about 69.4 x the capacity + 64 MiB) */
    /* the last LCP pass on this context (dk_dev_lcp and the other *_lcp entries) */
    uint64_t lcp_measured;        /* positions whose common prefix was measured, i.e. irreducible ones (counted only while profiling is enabled) ... */
    uint64_t lcp_bytes_compared;  /* ... and the bytes compared for them */
    uint32_t lcp_passes;          /* passes over the lists of long common prefixes: 1 unless a list was full */
} dk_stats;
#define DK_ROUTE_SHORT_PREFIX 0x1u      /* the prefix probe shortened the initial sort's key */
#define DK_ROUTE_NARROW_KEYS 0x2u       /* ... and its last pass left 32-bit keys */
#define DK_ROUTE_TEXT_ROUND 0x4u        /* a text-extension round ran */
#define DK_ROUTE_ISA_WINDOWS 0x8u       /* rank array through LDS windows */
#define DK_ROUTE_ISA_MARKED 0x10u       /* ... with the active suffixes' head positions handed over by marked SA entries */
#define DK_ROUTE_ISA_BUCKETS 0x20u      /* reserved (rounds 1-4: rank array by a bucketed store for blocks above 2^27 suffixes; every block goes through the windows now) */
#define DK_ROUTE_GENERAL_ROUND 0x40u    /* a doubling round in its general form ran */
#define DK_ROUTE_BIG_GROUPS 0x80u       /* ... with groups of more than 1024 members through the global sort */
#define DK_ROUTE_INPLACE_ROUNDS 0x100u  /* in-place (plateau) rounds ran */
#define DK_ROUTE_PAIR_CHAINS 0x200u     /* ... after pair chains settled groups of two to four */
#define DK_ROUTE_LFIRST 0x400u          /* BWT callers: only groups with different symbols in front were refined (no suffix array) */
#define DK_ROUTE_LFIRST_BIG_ROUND 0x800u  /* ... with at least one global-sort round of big groups */
#define DK_ROUTE_LFIRST_DEEP 0x1000u    /* ... and groups that went the way of long repeats (common extension measured directly) */
#define DK_ROUTE_LFIRST_GIANT 0x4000u    /* ... and common extensions longer than 64 KiB, measured by the whole grid (copies of whole files) */
#define DK_ROUTE_LFIRST_FALLBACK 0x2000u  /* the L-first path gave up: most of the block in big groups, giant groups, the round limit, two stalled
                                            rounds in a row, a full list (deep groups, their arena, the giant list or its arena) or a common
                                            extension still giant after the last giant round.  The suffix-array path, from the start */
#define DK_ROUTE_PERIOD_ROUND 0x8000u    /* a period round ran: suffixes inside stretches of one short period (runs, (ab)^n, zero padding) placed by where the stretch ends */
#define DK_ROUTE_PACKED_PAIRS 0x10000u   /* the initial sort moved packed pairs: key, carried code and position in one 64-bit word (at most 32 key bits, small alphabets) */
#define DK_ROUTE_PACKED_GUARD 0x20000u   /* packed path: at least one block was still unresolved after the pack's round limit and went through the single-block path */
#define DK_ROUTE_LCP_LONG 0x40000u       /* LCP pass: at least one position was still equal at the lane's cap (256 bytes) and went to the wave kernel */
#define DK_ROUTE_LCP_GIANT 0x80000u      /* ... and at least one was still equal at the wave's cap (64 KiB) and was measured by the whole grid */
/* enable (1) / disable (0) HIP-event bracketing of every kernel launch on the context's stream */
int dk_set_profiling(dk_ctx *ctx, int enabled);
int dk_stats_reset(dk_ctx *ctx);
int dk_get_stats(const dk_ctx *ctx, dk_stats *out);
/* name of kernel slot i (NULL past the end) */
const char *dk_kernel_name(int slot);

/* ---- host coding threads (operations; nothing in the reference corresponds: its coder is one thread) ------------------------------------
 * A large single block is coded by a pipeline of 2, 4, 5 or 6 host threads confined to one last-level-cache group; groups are
 * claimed per process, and a process that finds none free codes on one thread.  A launcher of several ranks per node can make that
 * deterministic: ask every rank how many groups it could claim, and set the same form everywhere. */
/* thread form of the host coding pass, process-wide: 0 automatic (default; or DK_ENTROPY_THREADS at load time) | 1 | 2 | 4 | 5.
 * 5 = the five-stage pipeline; for a stream of 2^21 distances or more, where the claimed L3 group has a sixth usable core, the same pipeline
 * with a sixth thread between the merger and the coder that prepares the coder's factors (six threads are reported).  Automatic takes the
 * same form under the same conditions.  Every form codes the same bytes. */
int dk_set_entropy_threads(int mode);
/* number of last-level-cache groups in which the calling thread may use at least min_cores cores */
int dk_host_l3_groups(int min_cores);
/* the calling thread's last host coding pass: threads used (1 / 2 / 4 / 5 / 6) and the L3 group claimed (-1: none).  Either may be NULL. */
void dk_last_entropy_info(int *threads, int *l3_group);
/* memory node the calling thread's coding passes should claim their L3 group on first (-1: none; the block entry points set it to their
 * context's GPU's node themselves -- for callers of dk_stream_encode that know where their staging memory lives) */
void dk_set_entropy_numa_node(int node);
/* the order in which a coding pass tries the machine's L3 groups, on a topology given by the caller (group_numa[g] = memory node of group g,
 * own = the caller's group, preferred_numa as above): indices into order_out[ngroups], returns how many.  For tests of the policy on
 * machines the test host is not (two sockets, eight GPUs). */
int dk_dbg_l3_claim_order(const int *group_numa, int ngroups, int own, int preferred_numa, int *order_out);

/* ---- stage-level debug entry points used by the parity tests ------------------------------------------------ */
/* dk_stream_encode on a distance stream that is still ARRIVING, the way dk_dev_block_encode feeds its host coder while the D2H copies
 * of a large block run: *ready (read atomically; another thread of the caller moves it) = entries of dist / sym that are there.  The
 * coder waits at that frontier; (size_t)-1 there = "the producer gave up", and a frontier that stands still for stall_ms milliseconds
 * (0 = 20 s) = "the stream hangs": DK_E_HIP in both cases instead of a coder that spins for ever.  host_threads: 0 automatic | 1 | 2 | 4 | 5. */
int dk_dbg_stream_encode_gated(int model_id, size_t n, const uint32_t init[256], const uint32_t *dist, const uint8_t *sym, size_t m,
                               uint32_t origin, uint8_t *out, size_t out_cap, size_t *out_len, const size_t *ready, unsigned stall_ms,
                               int host_threads);
/* stable LSD radix sort of (u64 key, u32 value) pairs on bits [begin_bit, end_bit) -- the workhorse of the suffix sort.  Exactly those bits: a
 * width that is no multiple of eight ends in a pass with a narrower digit, and what a key holds below begin_bit or from end_bit up travels with
 * its pair without a say in the order. */
int dk_dbg_sort_pairs(dk_ctx *ctx, uint64_t *keys, uint32_t *vals, size_t count, int begin_bit, int end_bit);
/* the same on device arrays, in place (measurement: tools/local_sort_bench.py) */
int dk_dbg_dev_sort_pairs(dk_ctx *ctx, uint64_t *d_keys, uint32_t *d_vals, size_t count, int begin_bit, int end_bit);
/* every 8192-pair tile of a device array sorted by itself inside one workgroup's LDS (the local pass an MSD-first sort would end with:
 * an experiment of round 4) */
int dk_dbg_dev_local_sort(dk_ctx *ctx, uint64_t *d_keys, uint32_t *d_vals, size_t count, int begin_bit, int end_bit);
/* ngroups independent stable sorts on bits [begin_bit, end_bit) in one launch per size class (the medium groups of the L-first path): group g is
 * the pairs [starts[g], starts[g + 1]) of d_kin / d_vin.  A group of more than `above` and at most 8192 pairs goes, sorted, to the same places
 * of d_kout / d_vout; nothing is written for any other group.  d_kout == d_kin and d_vout == d_vin (in place) are allowed.  `starts` is HOST
 * memory, ngroups + 1 entries: DK_E_ARG unless it is non-decreasing and ends at most at npairs. */
int dk_dbg_dev_sort_groups(dk_ctx *ctx, const uint64_t *d_kin, const uint32_t *d_vin, uint64_t *d_kout, uint32_t *d_vout, const uint32_t *starts,
                           size_t ngroups, size_t npairs, uint32_t above, int begin_bit, int end_bit);
/* One regrouping of the suffix sort on device arrays the caller built: rerank() (k_rerank_reduce, k_rerank_scan / _a / _c, k_rerank_apply or
 * k_rerank_apply_first) and the classification of the new groups behind it (k_big_reduce / _spine / _apply), with the mailbox read back as the
 * sort reads it.  A full context only.  tests/rerank_model.py is the definition of every output.
 *   d_keys, key_bytes   `count` sorted keys of 8 or 4 bytes (naturally aligned).  4: the narrow first rerank, with d_bucket_starts[256] (slots that
 *                       are heads whatever their words say; values from `count` up name no slot); otherwise d_bucket_starts is null
 *   d_idx, d_pos_in     the suffix and the SA position of every slot.  d_pos_in null: the FIRST rerank (slot a is SA position a; finals are left
 *                       where they stand, so d_sa, d_sym_in and d_origin are not looked at and d_bwt is read, L[a] being slot a's symbol)
 *   d_gid_in            (may be null) the group every slot was in before: a head wherever it changes, and such heads keep their members' ranks
 *   cmp_shift           low key bits outside the comparison; only the first rerank of 8-byte keys has any, 0 everywhere else
 *   d_rank, d_sa        (either may be null) later reranks: rank[idx] = SA position of the group's head; sa[pos] = idx for finals
 *   d_bwt, d_sym_in, d_sym_out, d_origin   the carry (d_bwt null: none; otherwise d_sym_out, and in a later rerank all four)
 *   d_out_idx, d_out_pos, d_out_gid        the new active list; d_gstart (count / 2 + 1 words); d_bigidx, d_bigoff (count / 2 words each)
 *   ls_max              groups of more members are big
 *   counts_out          (host) active, groups, big_slots, big_groups, above_pl_slots
 *   reduce_tiles_per_wg, first_tiles_per_wg, sparse_max   the launch shapes of k_rerank_reduce and k_rerank_apply_first: 1 .. 64 tiles per
 *                       workgroup and 0 .. 2048 survivors up to which a tile is fetched slot by slot; 0, 0 and a negative number = what the sort
 *                       itself takes.  The outputs do not depend on them.
 * The caller's duties are the sort's own: idx[a] < the length of d_rank, pos_in[a] < the length of d_sa and d_bwt, and arrays of the sizes above.
 * DK_E_ARG before anything is launched: a null context or array, an open batch, count == 0 or above the context's capacity or 2^31 - 2, other key
 * sizes, 4-byte keys with d_pos_in or d_gid_in or without bucket starts, d_rank without d_pos_in, a cmp_shift where there is none, half a carry,
 * more than 64 tiles per workgroup, sparse_max above 2048.  DK_E_NOMEM when rerank()'s workspace (1.01 bytes per slot) does not fit. */
int dk_dbg_dev_rerank(dk_ctx *ctx, const void *d_keys, int key_bytes, const uint32_t *d_bucket_starts, const uint32_t *d_idx, const uint32_t *d_pos_in,
                      const uint32_t *d_gid_in, int cmp_shift, size_t count, uint32_t *d_rank, uint32_t *d_sa, uint8_t *d_bwt, const uint8_t *d_sym_in,
                      uint8_t *d_sym_out, uint32_t *d_origin, uint32_t *d_out_idx, uint32_t *d_out_pos, uint32_t *d_out_gid, uint32_t *d_gstart,
                      uint32_t *d_bigidx, uint32_t *d_bigoff, uint32_t ls_max, uint32_t counts_out[5], unsigned reduce_tiles_per_wg,
                      unsigned first_tiles_per_wg, int sparse_max);
/* One rerank of the L-first path on device arrays the caller built: lf_rerank() of csrc/lfirst.inc (k_lf_reduce<u64 | u32>, k_lf_straddle, the scan
 * k_rerank_scan / _a / _c, k_lf_apply) and the classification of the live groups behind it as the path runs it after its first rerank, with the
 * mailbox read back as the path reads it.  A full context only.  tests/lf_rerank_model.py is the definition of every output.  The rules:
 *   heads     slot 0; every slot whose compared key bits differ from the slot's in front (8-byte keys: the bits from cmp_shift up; 4-byte keys:
 *             the whole word); with d_bucket_starts every slot that one of its 256 words names (values from `count` up name no slot)
 *   live      a group (a head's slot up to the next head) is LIVE iff it has more than one member and (two different symbols in front, or suffix
 *             0 among its members: the slot *d_zero_slot where that is given, the slot with d_idx == 0 otherwise).  Every other slot is FINAL
 *   list      the live slots in slot order: d_out_idx = d_idx, d_out_pos = d_pos_in (null: the slot number), d_out_gid = the live groups in
 *             front of the slot's group, d_out_sym = its symbol; d_gstart[g] = the list place of live group g's head, d_gstart[groups] = active
 *   depths    d_gdepth_out (may be null: nothing is written) per live group: depth_uniform, or with d_bigdepth (the big-list rule)
 *             d_bigdepth[key of the group's head >> key_shift] + depth_add.  (The rule's token fields are left out: no next-break positions.)
 *   finals    d_pos_in given (a LATER rerank): d_bwt[d_pos_in] = the slot's symbol, *d_origin = d_pos_in where d_idx == 0.  d_pos_in null
 *             (the FIRST rerank: slot a is SA position a and L holds its symbol already): nothing is written to d_bwt or d_origin
 *   symbols   sym_from_key (8-byte keys): a slot's symbol is its key's low byte, and d_sym holds those bytes afterwards; otherwise d_sym is read
 *   counts_out (host) active, groups, and the slots and groups of the big groups: more than 256 members (the tuning build's DK_LF_MAX lowers it)
 *   reduce_tiles_per_wg   tiles a workgroup of k_lf_reduce takes: 1 .. 64, 0 = what the sort takes (ntiles / 16384, so 1 below 2^25 slots).  The
 *                         outputs do not depend on it.
 * Everything else stays as it was: the lists from `active` on, d_gstart from groups + 1 on, d_gdepth_out from `groups` on, d_bwt at the places of
 * live slots, the origin word unless suffix 0 is final.  The caller's duties: arrays of `count` entries (d_gstart: count / 2 + 1 words,
 * d_gdepth_out: count / 2), d_pos_in[a] below the length of d_bwt, with d_bigdepth every key >> key_shift below its length.
 * DK_E_ARG before anything is launched: a null context or array (d_bucket_starts, d_zero_slot, d_pos_in, d_gdepth_out, d_bigdepth may be null;
 * d_bwt and d_origin in the first rerank), an open batch, count == 0 or above the context's capacity or 2^31 - 2, other key sizes, bucket starts
 * with 8-byte keys, a cmp_shift outside 0 .. 63 or with 4-byte keys, sym_from_key with 4-byte keys, d_bigdepth with 4-byte keys or without
 * d_gdepth_out or with a key_shift outside 0 .. 63, more than 64 tiles per workgroup.  DK_E_NOMEM when the workspace (3.2 bytes per slot) does not fit. */
int dk_dbg_dev_lf_rerank(dk_ctx *ctx, const void *d_keys, int key_bytes, const uint32_t *d_bucket_starts, int cmp_shift, uint8_t *d_sym, int sym_from_key,
                         const uint32_t *d_idx, const uint32_t *d_zero_slot, const uint32_t *d_pos_in, size_t count, uint32_t *d_out_idx, uint32_t *d_out_pos,
                         uint32_t *d_out_gid, uint8_t *d_out_sym, uint32_t *d_gstart, uint8_t *d_bwt, uint32_t *d_origin, uint32_t *d_gdepth_out,
                         uint32_t depth_uniform, const uint32_t *d_bigdepth, int key_shift, uint32_t depth_add, uint32_t counts_out[4],
                         unsigned reduce_tiles_per_wg);
/* The refinement of the L-first path from a list the caller built, to its end: lfirst_path() of csrc/lfirst.inc in its take-over form -- the filter
 * (lf_rerank on the group ids), k_lf_finish, the big rounds (global and grouped sorts, lf_rerank, k_lf_medium) and the passes over the deep groups
 * (k_lf_deep_wave, k_lf_deep_block, k_lf_lce) -- with the sort's own buffers for n from the workspace.  A full context only.  The tuning build's
 * DK_LF_* knobs act as in dk_dev_bwt_forward.  tests/lf_refine_model.py is the definition of the outputs:
 *   the list   `count` <= n slots: the suffix d_idx[a] (< n, distinct), its place d_pos[a] in L (< n, distinct), its group d_gid[a] (a group is a run
 *              of equal words) and the symbol in front d_sym[a].  The members of a group are equal in their first h0 symbols (the caller's duty)
 *   L          for every group: its members ordered by their suffixes (plain byte comparison, a proper prefix is smaller), its places taken in
 *              list order; d_bwt[k-th place] = d_sym of the k-th smallest member.  *d_origin = the place of suffix 0 if it is listed.  Every other
 *              byte of d_bwt (n bytes) and the origin word stay as they were.  No kernel derives a symbol from the text: d_sym is a free label
 *   period     0: no tokens.  1 .. h0: the text's short period; big groups whose members follow it through their depth are keyed by where their
 *              stretch ends (DK_ROUTE_PERIOD_ROUND), from the first round on; the n words of next-break room come from the workspace
 *   out        (host, 8 words) the verdict: 1 = L is complete, 2 = the path gave up half way (L has been written to, at listed places only; the
 *              sort would start over without it) | DK_ROUTE_* bits | rounds (k_lf_finish launches) | and the path's counters as its last kernel left
 *              them: entries of the deep list | members in the deep groups' arena | subgroups on giant list 0 | the give-up word | giant list 1
 * DK_E_ARG before anything is launched: a null context or pointer, an open batch, n below 64 or above the context's capacity, count == 0 or above n,
 * h0 == 0 or above n, a period below 0 or above h0.  DK_E_NOMEM when the sort's workspace for n (and 4 n bytes with a period) does not fit. */
int dk_dbg_dev_lf_refine(dk_ctx *ctx, const uint8_t *d_text, size_t n, const uint32_t *d_idx, const uint32_t *d_pos, const uint32_t *d_gid, const uint8_t *d_sym,
                         size_t count, uint32_t h0, int period, uint8_t *d_bwt, uint32_t *d_origin, uint32_t out[8]);
/* The last stage of the suffix-array path on a list the caller built: in_place_rounds() of csrc/suffix_array.hip -- k_to_inplace, the pair chains
 * (k_chain_extract, the record sort, k_chain_ends / _tiles / _spine / _verdicts / _apply), the in-place rounds (k_plateau_sort, k_plateau_ranks) and the
 * compaction (k_plateau_count / _scan / _compact) -- with the sort's own buffers for n from the workspace.  A full context only.  None of these
 * kernels reads the text: they work from the ranks, the list and h.  tests/in_place_model.py is the definition of every output.
 *   n, h        the text's length and the depth the members of a group are equal to (the kernels get min(h, n))
 *   the list    `count` slots: the suffix d_idx[a] and its SA position d_pos[a]; d_gid[a] = the slot's group and d_gstart[g] = the group's first
 *               slot, d_gstart[groups] = count: the format rerank writes, which k_to_inplace reads
 *   d_rank      n words, in and out: rank[x] = the SA position of the head of x's group (of x itself where x is final)
 *   the mode    d_sa (n words): finals are written as sa[position] = suffix.  Or d_bwt (n bytes) with d_sym (the symbol in front of every slot), d_origin
 *               and d_out_sym: finals are written as bwt[position] = symbol, *d_origin = the position of suffix 0 when it becomes final.  The symbol is
 *               a free label: no kernel here derives it from the text.  In the d_sa mode there is no origin word
 *   chain_group    0: no pair chains; 2 .. 4: groups of up to that many members get records (1 counts as 2); negative: the sort's own
 *   record_cap     0: n, as in the sort; otherwise the records k_chain_extract may reserve (what does not fit stays with the rounds)
 *   max_rounds     negative: to the end; k: at most k rounds are launched and waited for; 0: k_to_inplace and the chains only
 *   always_compact 0: as the sort decides; 1: a compaction behind the chains and behind every round read while slots are alive, whatever the counts
 *   the list afterwards   d_out_idx, d_out_meta, d_out_pos (d_out_sym): out[0] entries of the set the last round or compaction wrote -- a suffix with
 *               bit 31 set is final since the last round, 0xFFFFFFFF since longer; meta = offset in the group | (size - 1) << 8 | moved << 16; meta and
 *               sym mean something in live slots only.  Nothing is copied when no slot is alive (out[1] == 0): nobody reads the list again
 *   out         (host, 8 words) slots | live slots | chain records | 1 = the record list was full | slots the chains settled | rounds launched |
 *               compactions | DK_ROUTE_* bits
 * The caller's duties: every group has at most 256 members; the members of a group are equal in their first h symbols (so each has h symbols);
 * d_rank as above for EVERY suffix of the text; d_idx distinct and below n, d_pos distinct and below n; output arrays of `count` entries.
 * DK_E_ARG before anything is launched: a null context or pointer, both modes or neither (or half of the second), an open batch, n below 2 or above
 * the context's capacity, count == 0 or above n, groups == 0 or above count or n / 2 + 1, h == 0, chain_group above 4, record_cap above n.
 * DK_E_NOMEM when the sort's workspace for n does not fit. */
int dk_dbg_dev_in_place(dk_ctx *ctx, size_t n, uint32_t h, size_t count, const uint32_t *d_idx, const uint32_t *d_pos, const uint32_t *d_gid, const uint32_t *d_gstart,
                        size_t groups, uint32_t *d_rank, uint32_t *d_sa, uint8_t *d_bwt, const uint8_t *d_sym, uint32_t *d_origin, int chain_group, uint32_t record_cap,
                        int max_rounds, int always_compact, uint32_t *d_out_idx, uint32_t *d_out_meta, uint8_t *d_out_sym, uint32_t *d_out_pos, uint32_t out[8]);
/* One general round of the suffix sort on a list the caller built: general_round() of csrc/suffix_array.hip -- k_round_local<false> / <true>, the big
 * list through the global sort, k_big_back, then the rerank and the classification behind it -- with the sort's own buffers for n from the
 * workspace and the caller's groups classified by the sort's own classify_and_read.  A full context only.  tests/round_model.py is the definition
 * of every output.
 *   d_text, n, h   the text and the depth the members of a group are equal to (the kernels get min(h, n))
 *   the list    `count` slots in the format rerank writes: the suffix d_idx[a], its SA position d_pos[a], d_gid[a] = the slot's group, d_gstart[g] =
 *               the group's first slot, d_gstart[groups] = count
 *   d_rank      n words, in and out; needed when tsym == 0, optional otherwise (null: no ranks exist yet, as in the sort's text rounds):
 *               rank[x] = the SA position of the head of x's group (of x itself where x is final)
 *   tsym        0: a doubling round, the secondary key is the rank h further on.  Above 0: a text round of that many symbols behind the first h; the
 *               entry reads the alphabet as the sort does and takes raw bytes (eight of them, whatever tsym) from 17 byte values on, else coded
 *               symbols, at most as many as 63 bits hold
 *   period, d_next_break   period > 0 (with tsym == 8): a token round -- the members of a group that follows the period through its first h symbols
 *               are keyed by where their stretch ends; d_next_break (n words) is the caller's: nb[i] = min{j >= i: j + period >= n or T[j] != T[j + period]}
 *   the mode    d_sa (n words): finals are written as sa[position] = suffix.  Or d_bwt (n bytes) with d_sym (the symbol in front of every slot), d_origin,
 *               d_out_sorted_sym and d_out_sym: finals are written as bwt[position] = symbol, *d_origin = the position of suffix 0 when it becomes
 *               final.  The symbol is a free label wherever the big list's keys have room for it (always, below 2^40 bytes of text)
 *   the sorted state   d_out_sorted_keys, d_out_sorted_idx (d_out_sorted_sym): `count` entries, every group sorted inside its own slot range by its
 *               secondary key, ties in slot order; the key of a member of a big group is its group's index among the big groups << kb | the
 *               leading kb bits of its secondary key
 *   the next list      d_out_idx, d_out_pos, d_out_gid (d_out_sym): out[0] entries; d_out_gstart: out[1] + 1 entries
 *   out         (host, 8 words) slots of the next list | its groups | slots in its groups above 1024 | those groups | slots in groups above 256 |
 *               symbols the round advanced the depth by | DK_ROUTE_* bits | kb
 * The caller's duties: the members of a group are equal in their first h symbols; d_idx distinct and below n, d_pos distinct and below n; d_gid and
 * d_gstart as above; d_rank as above for EVERY suffix of the text; d_next_break as above; output arrays of `count` entries (gstart: count / 2 + 2).
 * DK_E_ARG before anything is launched: a null context or pointer, both modes or neither (or part of the second), an open batch, n below 2 or above
 * the context's capacity, count == 0 or above n, groups == 0 or above count or n / 2 + 1, h == 0, tsym below 0 or above 63, tsym == 0 without
 * d_rank, a period below 0 or above h or 2^18, a period without d_next_break or the reverse, a period with a tsym other than 8.
 * DK_E_NOMEM when the sort's workspace for n does not fit. */
int dk_dbg_dev_round(dk_ctx *ctx, const uint8_t *d_text, size_t n, uint32_t h, size_t count, const uint32_t *d_idx, const uint32_t *d_pos, const uint32_t *d_gid,
                     const uint32_t *d_gstart, size_t groups, uint32_t *d_rank, int tsym, int period, const uint32_t *d_next_break, uint32_t *d_sa, uint8_t *d_bwt,
                     const uint8_t *d_sym, uint32_t *d_origin, uint64_t *d_out_sorted_keys, uint32_t *d_out_sorted_idx, uint8_t *d_out_sorted_sym, uint32_t *d_out_idx,
                     uint32_t *d_out_pos, uint32_t *d_out_gid, uint32_t *d_out_gstart, uint8_t *d_out_sym, uint32_t out[8]);
/* The period kernels and the text probes of the suffix sort on the caller's text, through the launches the sort's phases use but without their size
 * thresholds.  A full context only.  d_text may have any alignment.  Every part is optional and switched on by its argument; the outputs other than
 * d_next_break are host arrays.  tests/period_model.py is the definition of every output.
 *   period, d_next_break   period > 0: k_period_first / _spine / _fill; d_next_break[i] (n words) = min{j >= i: j + period >= n or T[j] != T[j + period]}
 *   run_out[2]     k_run_probe: [0] = 1 when an aligned 256-byte window of one byte value exists, [1] = 16-byte pieces of one value in whole windows
 *   probe_out[8]   k_period_probe: [p - 1] = the 64-byte windows w with 64 w + 72 <= n that follow period p
 *                  (a d_text that is not 16-byte / 8-byte aligned forgoes these two verdicts: all zero)
 *   count_p, count_out     k_period_count: the 64-byte windows w with 64 w + 64 + count_p <= n that follow period count_p
 *   search_pmax, found_out[32]   k_period_search: per sample position x = (2 b + 1) n / 64 the smallest p in [9, search_pmax] with 48 equal bytes
 *                  at x and x + p; 0xFFFFFFFF: none, or x + search_pmax + 48 > n
 *   m, span, cands, ncands, dups_out[4]   k_prefix_probe: m samples a span apart (jittered by a hash of the sample's number), ncands prefix
 *                  lengths in symbols of the code the entry reads from the text as the sort does; dups_out[c] = samples minus distinct prefixes
 *                  of cands[c] symbols ([ncands, 4): zero)
 * DK_E_ARG before anything is launched: a null context or text, an open batch, n == 0 or above the context's capacity, a period below 0 or above
 * 2^18, an argument of a part without its output or the reverse, search_pmax outside 9 .. 2^18, ncands outside 1 .. 4, m == 0 or above n or 2^24,
 * span == 0, no part at all.  DK_E_ARG once the alphabet has been read: a candidate below 1 symbol, above what a key holds, or above 56 bits.
 * DK_E_NOMEM when n / 4096 words or the probe's table (the power of two from 2 ncands m on, 8 bytes each) do not fit. */
int dk_dbg_dev_period(dk_ctx *ctx, const uint8_t *d_text, size_t n, int period, uint32_t *d_next_break, uint32_t run_out[2], uint32_t probe_out[8], uint32_t count_p,
                      uint32_t *count_out, uint32_t search_pmax, uint32_t *found_out, uint32_t m, uint32_t span, const int *cands, int ncands, uint32_t dups_out[4]);
/* The initial sort of the suffix sort by itself: ONE sort_pairs() of csrc/radix_sort.hip with the text keys and the final destinations that
 * initial_sort() of csrc/suffix_array.hip hands it (both build them in one function) -- k_radix_hist<HS_TEXT>, the text pass of k_radix_scatter in its
 * plain and its packed form, the passes behind it and the last pass's stores to their final homes.  A full context only.  The alphabet is the
 * CALLER'S, not the one the sort reads from the text: no kernel of this stage derives one table from the other, so `code` may be non-injective
 * and `inv` is then any table.  tests/initial_sort_model.py is the definition of every output.
 *   d_text, n      the text; any alignment (only a 16-byte aligned text lets a tile take the 16-byte loads)
 *   code[256], bits, spk   (host) the code of every byte value, below 2^bits each; the window of position i = the codes of T[i .. i + spk) packed
 *                  big-endian, `bits` each, zero for positions from n on.  The tables go where the sort keeps them, the stages' mailbox
 *   inv[256], d_bwt, d_origin   the carry: all three or none.  With it the key of position i is window << 8 | code[T[i - 1]] (T[n - 1] for i = 0),
 *                  d_bwt[slot] = inv[key & 0xFF] (n bytes) and *d_origin = the slot of position 0; without it the key is the window
 *   narrow         1 (sorts of at most 40 bits): the last pass leaves 32-bit words, the window's low 32 bits; 0: the 64-bit keys
 *   the order      stable by window: an LSD sort on exactly the window's bits, ceil(bits spk / 8) passes, whose input stands in position order
 *   d_keys_out     n sorted keys, 8 bytes each or 4 when narrow, copied from whichever buffer of its pair the sort hands back
 *   d_sa           n words, written by the sort's last pass itself: the position at every slot
 *   bucket_starts_out[256]   (host; narrow only, null otherwise) [d] = the pairs whose last-pass digit -- the window's top bits, what the passes
 *                  before the last leave of it -- is below d: where two neighbours may differ in the bits a narrow word has lost
 *   out            (host, 4 words) the DK_ROUTE_* bits the sort set (DK_ROUTE_PACKED_PAIRS or none) | passes | pairs sorted over all passes, low word | 0
 * The four sort buffers (24 bytes per position) and the sort's tables come from the workspace, which is marked and released.
 * DK_E_ARG before anything is launched: a null context or array, an open batch, n == 0 or above the context's capacity or 2^31 - 2, bits outside
 * 1 .. 8, spk below 1 or bits spk + 8 (with the carry) above 64, a code[c] of more than `bits` bits (the packed word cannot hold it), half a carry,
 * narrow outside 0 / 1 or with more than 40 sorted bits, bucket_starts_out without narrow or the reverse.  DK_E_NOMEM when the workspace does not fit. */
int dk_dbg_dev_initial_sort(dk_ctx *ctx, const uint8_t *d_text, size_t n, const uint8_t code[256], int bits, int spk, const uint8_t inv[256], int narrow,
                            void *d_keys_out, uint32_t *d_sa, uint8_t *d_bwt, uint32_t *d_origin, uint32_t bucket_starts_out[256], uint32_t out[4]);
/* The segmented suffix sort of csrc/packed.hip one step at a time: the production sort is pk_first(), pk_round() until no
 * group is left or the round limit, and pk_guard(); these two entries run the same functions on their own.  A full context only.  The pack is
 * `count` blocks of n[i] bytes back to back, block i at [off_i, e_i), total = their sum; its limits are those of dk_dev_bwt_forward_packed.
 * tests/packed_round_model.py is the definition of every output.
 *
 * dk_dbg_dev_packed_first: k_pk_hist, k_pk_codes, k_pk_init_keys, their sort and the first regroup.
 *   code[256]      (host, out) code[c] = 1 + the present byte values below c, 0 for an absent c; sigma = the present values
 *   the key        block id, then k_used codes of `bits` bits, 0 from the block's end on; bits = max(1, ceil_log2(sigma + 1)),
 *                  blk_bits = ceil_log2(count), k_used = min(max(1, (64 - blk_bits) / bits), total)
 *   d_keys, d_vals total entries each: the keys in order and the position each belongs to; stable, so equal keys stand in position order
 *   d_rank         total words: d_rank[p] = the slot of the first member of p's group (the suffixes with p's key)
 *   d_act          total words, of which the first `live` are written and the rest left untouched: the members of groups of two or more,
 *                  in list order
 *   out            (host, 8 words) sigma | bits | blk_bits | k_used | live | the bit the sort ended at (blk_bits + bits k_used) | 0 | 0
 * DK_E_ARG before anything is launched: a null context or pointer, an open batch, a decoder context, a pack that dk_dev_bwt_forward_packed refuses.
 *
 * dk_dbg_dev_packed_round: k_pk_round_keys, the sort and the regroup (k_pk_tile_sum, k_pk_spine, k_pk_tile_apply) at depth h on a state the
 * CALLER built, and k_pk_guard_mark on the list it leaves.  The round reads no text, and the ranks need not come from one.
 *   d_act, c       the list: c distinct suffixes below total
 *   d_rank         total words, in and out; only the entries of listed suffixes change
 *   the key        d_rank[p] << rbits | rank2, rbits = ceil_log2(total + h), rank2 = d_rank[p + h] + h, or e_i - 1 - p when p + h >= e_i
 *   d_keys, d_vals c entries each: the round keys in order and their suffixes; stable, so equal keys keep the order of d_act
 *   the ranks      a member at list index k of an old group (the entries with one d_rank) that starts at list index ks and has the rank g gets
 *                  g + (list index of the first entry with its key - ks)
 *   d_next_act     c words, of which the first `live` are written: the entries whose key occurs twice or more, order kept
 *   d_guard        (may be null) count words: 1 where the block holds a suffix of the next list, else 0
 *   out            (host, 8 words) rbits | gbits = ceil_log2(total) | live | 0 ...
 * The caller's duties: the entries of d_act are distinct and below total; every d_rank[p] is below total, and d_rank[p] plus the number of listed
 * members of p's old group is at most total.
 * DK_E_ARG before anything is launched: a null context or required pointer, an open batch, a decoder context, a pack refused as above, c == 0 or
 * above total, h == 0 or above 2^31.
 * Both: the sort's buffers come from the workspace, which is marked and released; DK_E_NOMEM when they do not fit.  Both synchronise. */
int dk_dbg_dev_packed_first(dk_ctx *ctx, const uint8_t *d_text, size_t count, const size_t *n, uint64_t *d_keys, uint32_t *d_vals, uint32_t *d_rank,
                            uint32_t *d_act, uint16_t code[256], uint32_t out[8]);
int dk_dbg_dev_packed_round(dk_ctx *ctx, size_t count, const size_t *n, uint32_t h, const uint32_t *d_act, size_t c, uint32_t *d_rank, uint64_t *d_keys,
                            uint32_t *d_vals, uint32_t *d_next_act, uint32_t *d_guard, uint32_t out[8]);
/* d_rank[d_sa[p]] = p for a permutation d_sa of 0 .. n-1 (n <= 2^31), through LDS windows.  d_marked_val (may be null): an entry of d_sa with bit
 * 31 set stands for d_sa[p] & 0x7FFFFFFF and its value is d_marked_val[p] instead of p.  The two n-u64 scratch arrays come from the context's
 * workspace: DK_E_NOMEM when they do not fit.  What it does with an input that is no permutation is not defined beyond "no store outside d_rank". */
int dk_dbg_dev_inverse_permutation(dk_ctx *ctx, const uint32_t *d_sa, size_t n, uint32_t *d_rank, const uint32_t *d_marked_val);
/* The two instruments of tests/test_gpu_poison_stages.py and tests/test_gpu_call_sequences.py; both are served by a decoder context as well (any_ctx) and
 * return DK_E_ARG for a null context or while a streaming batch is open.
 * dk_dbg_mail_fill: every word of the stages' mailbox (csrc/mailbox.hpp), the device page and its pinned host twin, set to `byte` (0 .. 255) on the
 * context's stream, which is synchronised.  Between complete API calls only.  A stage that reads a word it has not cleared or written in its
 * own call then reads `byte` instead of what the call before it happened to leave (zeros on a fresh context). */
int dk_dbg_mail_fill(dk_ctx *any_ctx, int byte);
/* dk_dbg_ws_peek: nbytes (> 0; DK_E_NOMEM beyond the workspace) allocated from the workspace the way a stage allocates them, copied to host_out
 * before anything has written them, released.  In the tuning build under DK_POISON=<b> every byte comes back as b, whatever nbytes is and whatever
 * the call before left there: the proof that a poisoned run is poisoned.  In any other build the bytes are whatever the workspace holds. */
int dk_dbg_ws_peek(dk_ctx *any_ctx, size_t nbytes, uint8_t *host_out);

#ifdef __cplusplus
}
#endif
#endif /* DARK_AMD_H */
