// runner_internal.h — what the runner's three files share: sources and
// sinks, a slot's state and the runner itself.
//   runner.cpp         host pool, placement, create/destroy, the run loops
//   runner_decode.cpp  page loads and the device decode of a chunk's pages
//   runner_io.cpp      sources, sinks and the store side of every codec
#pragma once

#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>

#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "buffer.h"
#include "j2k.h"
#include "j2k_t1_lane.h"
#include "jpeg.h"
#include "pdf.h"
#include "runtime.h"
#include "tiff_dec.h"
#include "tiff_write.h"

namespace uph {

// Memory sources and sinks are page-locked (hipHostRegister) on their first
// run, so the runner's DMA copies read and write the caller's buffers
// directly instead of going through pinned staging and a host memcpy each way
// (image_pipeline.c:226-376 stages through pinned buffers because its decode
// produces frames in pageable memory).  Unregistered on destroy.
struct HostRegistration {
  void* ptr = nullptr;
  size_t bytes = 0;
  bool tried = false;
  bool ok = false;
  std::mutex mu;  // a source or sink may be shared by runners on other threads
  // Registers [p, p + n) once; n is the extent the runner reads or writes,
  // not a whole number of strides (the caller's last page need not be padded).
  bool ensure(const void* p, size_t n) {
    std::lock_guard<std::mutex> lk(mu);
    if (tried) return ok;
    tried = true;
    ok = hipHostRegister(const_cast<void*>(p), n, hipHostRegisterDefault) == hipSuccess;
    if (ok) {
      ptr = const_cast<void*>(p);
      bytes = n;
    } else {
      (void)hipGetLastError();  // registration is an optimisation: staged copies otherwise
    }
    return ok;
  }
  ~HostRegistration() {
    if (ok) hipHostUnregister(ptr);
  }
};

}  // namespace uph

struct UphipSource {
  UphipLoadFn load = nullptr;
  void* user = nullptr;
  // built-ins
  const uint8_t* base = nullptr;
  int64_t linesize = 0, page_stride = 0, npages = 0;
  std::vector<std::string> paths;
  // a PDF document: page i of it is input page i (uphip_source_pdf)
  std::shared_ptr<uph::pdf::Document> pdf;
  int32_t pdf_dpi = 0;
  // a multi-page TIFF: IFD i of it is input page i (uphip_source_tiff)
  std::shared_ptr<uph::tiff::Document> tiff;
  int32_t tiff_flags = 0;
  uph::HostRegistration reg;
};

struct UphipSink {
  // What the device makes of a chunk's sheets before they leave it:
  //   Raw   nothing: the sheets come back as they are (callback, memory, PNM, discard)
  //   Jpeg  JPEG files (uphip_sink_jpeg, uphip_sink_pdf fast)
  //   Jp2   lossless JPEG 2000 (uphip_sink_jp2, uphip_sink_pdf high): transforms and
  //         code-blocks on the device, packets on the store tasks
  //   G4    CCITT Group 4 streams of bilevel sheets (uphip_sink_tiff_g4: a TIFF per
  //         page, at pdf_dpi; uphip_sink_pdf_bilevel)
  //   Png   lossless zlib streams of sheets of any format (uphip_sink_png: a PNG per
  //         page, pHYs from png_dpi; uphip_sink_pdf_lossless)
  //   Tiff  TIFF pages in the runner's output format (uphip_sink_tiff: a file per
  //         page; uphip_sink_tiff_multipage: one file): Group 4 streams of
  //         MONOWHITE sheets, Deflate strips of GRAY8 and RGB24 sheets; the
  //         codec follows the format (packed_codec), resolution pdf_dpi
  enum class Codec { Raw, Jpeg, Jp2, G4, Png, Tiff };
  Codec codec = Codec::Raw;
  UphipStoreFn store = nullptr;
  void* user = nullptr;
  uint8_t* base = nullptr;
  int64_t linesize = 0, sheet_stride = 0, nsheets = 0;
  std::string pattern;
  int64_t wrap = 0;
  int32_t quality = UPHIP_JPEG_DEFAULT_QUALITY, sampling = UPHIP_JPEG_444;
  int32_t png_dpi = 0;
  // one PDF of all the output pages (uphip_sink_pdf*): the encoded pages go to
  // the writer instead of files
  std::unique_ptr<uph::pdf::Writer> pdfw;
  // one TIFF of all the output pages (uphip_sink_tiff_multipage)
  std::unique_ptr<uph::tiff::Writer> tiffw;
  int32_t pdf_dpi = 300;
  uph::HostRegistration reg;
};

namespace uph {

class HostPool;

// A JPEG page of a chunk: entropy-decoded by a load task into pinned memory
// (jpeg.h packed layout); the device thread uploads it and decodes it on the
// slot's stream straight into the batch's input slot before the run.
struct JpegPage {
  Buffer host{Buffer::Pinned};  // grown on demand
  bool on = false;              // this chunk's page is a JPEG waiting for the device
  bool dev = false;             // Huffman-decoded on the device (host holds a JdecHeader stream)
  size_t bytes = 0;             // bytes to upload
  JpegHeader h{};
  // a JPEG 2000 page instead: host holds its code-block jobs (j2k_t1_lane.h;
  // offsets relative to the page) then their codewords; the device decodes
  // the code-blocks of all the chunk's JPEG 2000 pages in one launch, then
  // runs each page's inverse transforms into its input slot
  bool j2k = false;
  j2k::Image img;
  int32_t njobs = 0;
  size_t jobs_bytes = 0;  // 256-aligned
  int maxw = 0, maxh = 0;
};

// A TIFF page of a chunk on the device route (tiff_dec.h): a load task
// leaves its blob (the strips' bytes, the palette) and its jobs (offsets
// relative to the page) in pinned memory; the device thread uploads the
// chunk's blobs and decodes all their strips in one launch on the slot's
// stream, then finishes the rows into the batch's input slots.
struct TiffPage {
  Buffer host{Buffer::Pinned};  // the blob; grown on demand
  bool on = false;              // this chunk's page waits for the device
  size_t bytes = 0;             // of the blob
  std::vector<tiff::StripJob> jobs;
  tiff::RowsPage rows{};
  uint64_t raster = 0;          // the page as stored: its share of the scratch
  bool lzw = false;
};

struct PageSize {
  int32_t w = 0, h = 0;
};

struct Slot {
  std::vector<JpegPage> jpg;     // per page of the chunk (sheet * input_count + page)
  std::vector<PageSize> psize;   // likewise: each page's own size (a fixed-sheet run places by it)
  std::vector<std::string> load_error;  // per sheet of the chunk: why its page did not load
  std::vector<TiffPage> tif;     // likewise
  Buffer dtif{Buffer::Device};   // the chunk's TIFF blobs, then its jobs and page records
  Buffer htif{Buffer::Pinned};   // the jobs and page records, offsets made chunk-wide
  Buffer dtsc{Buffer::Device};   // the decoded strips (every TIFF page as stored)
  Buffer dtpl{Buffer::Device};   // the LZW tables of k_tiff_strips' lanes (at most 64 MiB)
  Buffer dtst{Buffer::Device};   // per page: strip decode status (int32_t)
  bool tdev = false;             // the chunk has device-decoded TIFF pages (statuses to read)
  Buffer djpg{Buffer::Device};   // device copies of the chunk's packed JPEG pages
  Buffer hj2j{Buffer::Pinned};   // the chunk's JPEG 2000 jobs (j2k::T1Job), offsets made chunk-wide
  Buffer dj2j{Buffer::Device};   // their device copy
  Buffer dj2c{Buffer::Device};   // the JPEG 2000 pages' coefficient planes (uint32_t)
  Buffer dj2t{Buffer::Device};   // k_j2k_t1 scratch slots
  Buffer dscr{Buffer::Device};   // colour planes (one page at a time on the stream)
  Buffer djpk{Buffer::Device};   // packed coefficients of the device-decoded pages
  Buffer djsc{Buffer::Device};   // their device Huffman scratch
  Buffer djst{Buffer::Device};   // per page: device Huffman status (int32_t)
  Buffer djob{Buffer::Device};   // the decode jobs (JdecJob) and their pinned source
  Buffer hjob{Buffer::Pinned};
  bool jdev = false;             // the chunk has device-decoded pages (statuses to read)
  UphipBatch* b = nullptr;
  Buffer hin{Buffer::Pinned};    // input staging (count * input_count pages)
  Buffer hout{Buffer::Pinned};   // output staging (count sheets)
  Buffer din{Buffer::Device};    // device copy of a registered memory source's chunk
  bool direct_out = false;       // this chunk's D2H went straight into the sink
  int64_t first = 0;             // first job of the chunk in flight
  int32_t count = 0;
  int64_t last_first = -1;       // the chunk whose outputs the batch holds (uphip_runner_slot_chunk)
  int32_t last_count = 0;
  std::vector<char> failed;      // per sheet of the chunk: 1 device, 2 store, 4 load
  // packed codecs: the chunk's packed files and each page's size / offset
  Buffer hjpg{Buffer::Pinned};
  std::vector<int64_t> jsize, joff;
  // JPEG 2000 sink: the chunk's pages coded on the device (jp2_chunk_submit):
  // one device arena (coefficients and code-block outputs of a sub-batch,
  // the coder's slots, jobs, lengths, offsets, planes, packed codewords)
  // and the pinned copies of the offsets / lengths / planes per job
  Buffer dj2e{Buffer::Device};
  Buffer hj2e{Buffer::Pinned};
  j2k::Image j2img;
  int32_t j2jobs = 0;              // code-blocks a page
  uint32_t* hj2off = nullptr;      // views into hj2e (npages * j2jobs + 1, ...)
  uint32_t* hj2len = nullptr;
  uint8_t* hj2nb = nullptr;
  int32_t* hj2err = nullptr;
  const uint8_t* dj2pk = nullptr;  // packed codewords (device)
};

struct DeviceCtx {
  int device = 0;
  std::vector<Slot> slots;
  // placement (image_pipeline.c:226-376 sizes pools per device; here each
  // device also gets its node's CPUs): the device thread and this device's
  // load/store pool run on the CPUs of the GPU's NUMA node; pinned staging
  // comes from hipHostMalloc, which places it on the node nearest the
  // current device
  int numa = -1;
  bool pinned = false;
  cpu_set_t cpus;
  HostPool* pool = nullptr;
  void bind() const {
    if (pinned) pthread_setaffinity_np(pthread_self(), sizeof(cpus), &cpus);
  }
  // per-run results
  int64_t done = 0, failed = 0;
  double busy_s = 0;
  std::string error;
};

}  // namespace uph

struct UphipRunner {
  UphipOptions opts;
  UphipBatchGeometry geo;  // capacity = sheets per batch
  UphipRunnerConfig cfg;
  std::vector<int> devices;
  std::vector<uph::DeviceCtx> dev;
  int oc = 1;  // output pages a sheet
  int32_t out_w = 0, out_h = 0, out_fmt = 0;
  int64_t in_pitch = 0, in_page_stride = 0;   // batch input slot layout (= staging layout)
  int64_t out_linesize = 0, out_sheet_stride = 0;
  bool staged = false;  // pinned staging allocated
  // sheet_size fully set and no pre_rotate: geo's page size is the maximum, a
  // page of the format and at most that size is centred in the sheet
  bool fixed_sheet = false;
  int64_t batch_bytes = 0;  // device memory of one batch
  UphipRunnerStats stats{};
};

namespace uph {

// One entry per codec whose pages come back as one packed download (JPEG,
// Group 4, PNG).  A new codec of this shape is a new entry in runner_io.cpp.
struct PackedCodec {
  // queue the encode of the batch's finished run on its stream; 0 or -1
  int (*encode)(UphipBatch* b, const UphipSink* k);
  // each page's size (-1: larger than its share) and their total, or -1
  int64_t (*sizes)(UphipBatch* b, int64_t* sizes, int32_t max_pages);
  // queue the packed pages' copy into `host`; 0 or -1
  int (*download)(UphipBatch* b, void* host, int64_t capacity);
  // output page j of sheet s of the slot's chunk into the sink: from the
  // packed download, or -- a page of size -1 -- encoded again on its own
  bool (*store_page)(UphipRunner* r, const UphipSink* k, int device, const Slot* sl, int s, int j);
};
// null for Raw and Jp2; a Tiff sink's codec follows the runner's output
// format: Group 4 for MONOWHITE sheets, Deflate strips otherwise
const PackedCodec* packed_codec(const UphipSink* k, int32_t out_fmt);

// runner_io.cpp
void store_chunk_sheet(UphipRunner* r, const UphipSink* k, int device, const Slot* sl, int s, bool* ok);
bool sink_write(const UphipSink* k, int64_t idx, const uint8_t* p, size_t n, int32_t w = 0, int32_t h = 0);

// runner_decode.cpp
bool load_page(UphipRunner* r, int device, const UphipSource* s, int64_t job, int32_t j, uint8_t* dst,
               JpegPage* jp, TiffPage* tp, PageSize* ps);
// page idx of a PNM-list, TIFF or PDF source from its header, and a name for it
bool source_page_info(const UphipSource* s, int64_t idx, UphipPnmInfo* g, std::string* name);
bool upload_staging(UphipRunner* r, Slot* sl, int npages);
bool jpeg_submit(Slot* sl, int npages);
bool tiff_submit(Slot* sl, int npages);
bool jp2_chunk_submit(UphipRunner* r, Slot* sl, int npg);

}  // namespace uph
