// capi_internal.hpp -- everything the C-ABI translation units share (capi_open.hip, capi_extract.hip, capi_query.hip, capi_graph.hip, capi_topology.hip, capi_refpos.hip, capi_locate.hip, capi_build.hip, capi_gfa_build.hip, capi_merge.hip, capi_remove.hip, capi_lines.hip, capi_sequences.hip, capi_tags.hip, capi_suffix_array.hip, capi_fm.hip, capi_fm_seeds.hip, open_lines.hip, sequences.hip, suffix_array.hip, comm.hip), one header per concern:
#pragma once

#include "capi_status.hpp"     // statuses, HIP_CHECK, the guards of an entry point
#include "device_buffer.hpp"   // DeviceBuffer and where its memory lies
#include "knobs.hpp"           // the settings of an open and of a workspace
#include "hip_raii.hpp"        // stream, events, pinned words
#include "request_key.hpp"     // the memo of a request family
#include "handle.hpp"          // gbwt_hip_index
#include "workspace.hpp"       // gbwt_hip_workspace
#include "labels.hpp"          // the labels of a handle as kernels see them
