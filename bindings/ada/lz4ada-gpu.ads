-- lz4ada-gpu.ads -- bulk entry points of the GPU hot path (no reference
-- twin: SURVEY 8b "a per-block Update cannot reach the roofline").
-- A caller such as tool_unlz4ada can replace its Update loop for a whole
-- frame by one Decode_Frame call.  UNTESTED (no GNAT in this image).
with Interfaces;
with System;

package LZ4Ada.GPU is

	-- include/lz4ada_hip.h: lz4ada_decode_frame.  Raises the reference
	-- exception with the reference message on failure.
	procedure Decode_Frame(Frame:          in     Octets;
				Output:         in out Octets;
				Output_Length:  out    Interfaces.Integer_64;
				Frame_Consumed: out    Interfaces.Integer_64);

	-- lz4ada_decode_stream: every frame of a concatenated stream.
	procedure Decode_Stream(Input:         in     Octets;
				Output:        in out Octets;
				Output_Length: out    Interfaces.Integer_64);

	-- lz4ada_decoded_bound: output capacity needed by Decode_Stream.
	function Decoded_Bound(Input: in Octets) return Interfaces.Integer_64;

	-- lz4ada_decode_frame_multi: Decode_Frame over GPUs 0 .. N_GPUs-1 of
	-- this process (one host thread per device, RCCL for the verdict);
	-- frames that do not shard decode on GPU 0.  Same exceptions.
	procedure Decode_Frame_Multi(Frame:          in     Octets;
				N_GPUs:         in     Positive;
				Output:         in out Octets;
				Output_Length:  out    Interfaces.Integer_64;
				Frame_Consumed: out    Interfaces.Integer_64);

	-- lz4ada_decode_frames: many independent frames in as few device
	-- passes as the byte budget allows, a result per frame (lz4ada_frame_job
	-- of include/lz4ada_hip.h).  The caller fills Frame and Len; every
	-- other component is output.  Status is the lz4ada_status of that frame
	-- alone (0: decoded; Frames_Error gives the reference's message
	-- otherwise), so one bad frame does not cost the others.
	type Frame_Job is record
		Frame:    System.Address;
		Len:      Interfaces.Integer_64;
		Out_Off:  Interfaces.Integer_64;
		Out_Len:  Interfaces.Integer_64;
		Consumed: Interfaces.Integer_64;
		Status:   Interfaces.Integer_32;
		Path:     Interfaces.Integer_32;
	end record;
	pragma Convention(C, Frame_Job);
	type Frame_Jobs is array(Positive range <>) of aliased Frame_Job;
	pragma Convention(C, Frame_Jobs);

	-- Raises only when the call itself failed.  Output is allocated by the
	-- library (Output_Length bytes, every job's bytes at its Out_Off);
	-- release it with Buffer_Free.
	-- Linked: lz4ada_decode_frames_opt with LZ4ADA_FRAMES_LINKED -- linked
	-- frames up to Batch_Linked_Max share the passes (one wave per frame).
	procedure Decode_Frames(Jobs:          in out Frame_Jobs;
				Output:        out    System.Address;
				Output_Length: out    Interfaces.Integer_64;
				Linked:        in     Boolean := False);
	-- lz4ada_batch_linked_max: the slot bytes up to which a linked frame
	-- shares a pass (LZ4ADA_BATCH_LINKED_MAX overrides the default).
	function Batch_Linked_Max return Interfaces.Integer_64;
	pragma Import(C, Batch_Linked_Max, "lz4ada_batch_linked_max");
	-- lz4ada_frames_error: the message of job I (Jobs'First based) of the
	-- last Decode_Frames call of this task's thread.
	function Frames_Error(Jobs: in Frame_Jobs; I: in Positive) return String;
	procedure Buffer_Free(P: in System.Address);
	pragma Import(C, Buffer_Free, "lz4ada_buffer_free");

	-- lz4ada_frames_device_bound / lz4ada_decode_frames_device: many frames
	-- that already lie in device memory, decoded into device memory
	-- (lz4ada_device_frame_job of include/lz4ada_hip.h).  D_In and D_Out
	-- are device addresses, Stream a hipStream_t (Null_Address: the default
	-- stream).  The caller fills In_Off and In_Len; every other component
	-- is output.  Status is 0, or 9 (LZ4ADA_EXACT_PATH) with a Reason
	-- (LZ4ADA_DEVFRAME_*) for a frame the pass did not decode: Decode_Frame
	-- on that frame's host bytes gives the reference's result.
	type Device_Frame_Job is record
		In_Off:   Interfaces.Integer_64;
		In_Len:   Interfaces.Integer_64;
		Out_Off:  Interfaces.Integer_64;
		Out_Len:  Interfaces.Integer_64;
		Consumed: Interfaces.Integer_64;
		Status:   Interfaces.Integer_32;
		Reason:   Interfaces.Integer_32;
	end record;
	pragma Convention(C, Device_Frame_Job);
	type Device_Frame_Jobs is array(Positive range <>) of aliased Device_Frame_Job;
	pragma Convention(C, Device_Frame_Jobs);

	-- An output capacity that always suffices.  Raises only when the call
	-- itself failed (Program_Error: ranges that overlap or leave the input).
	function Frames_Device_Bound(D_In:   in     System.Address;
				In_Len: in     Interfaces.Integer_64;
				Jobs:   in out Device_Frame_Jobs;
				Stream: in     System.Address := System.Null_Address;
				Linked: in     Boolean := False)
				return Interfaces.Integer_64;
	-- lz4ada_frames_device_sizes: the exact decoded sizes, found on the
	-- device without decoding.  Out_Len of every accepted job is its frame's
	-- decoded length; the result is their sum, an output capacity that
	-- suffices for Decode_Frames_Device with Exact.  Status 9 with Reason 5
	-- or 6 (LZ4ADA_DEVFRAME_BLOCK / _SIZE): the sizes already fail the frame.
	function Frames_Device_Sizes(D_In:   in     System.Address;
				In_Len: in     Interfaces.Integer_64;
				Jobs:   in out Device_Frame_Jobs;
				Stream: in     System.Address := System.Null_Address;
				Linked: in     Boolean := False)
				return Interfaces.Integer_64;
	-- Too_Little_Memory when Out_Cap is below the bound (Output_Length then
	-- holds the bound and D_Out is untouched).  Exact: LZ4ADA_FRAMES_EXACT --
	-- the frames are sized first and laid out by their sizes, and the bound
	-- is Frames_Device_Sizes' total (the flags are then given as they stand:
	-- LZ4ADA_BATCH_LINKED in the environment is not consulted).
	procedure Decode_Frames_Device(D_In:          in     System.Address;
				In_Len:        in     Interfaces.Integer_64;
				Jobs:          in out Device_Frame_Jobs;
				D_Out:         in     System.Address;
				Out_Cap:       in     Interfaces.Integer_64;
				Output_Length: out    Interfaces.Integer_64;
				Stream:        in     System.Address := System.Null_Address;
				Linked:        in     Boolean := False;
				Exact:         in     Boolean := False);

	-- lz4ada_frames_device_bound_dict / lz4ada_decode_frames_device_dict:
	-- the two device calls with one dictionary in device memory that every
	-- frame of the call shares (lz4ada_device_dict of include/lz4ada_hip.h;
	-- the LZ4 specification's semantics, no reference twin).  The thin
	-- imports: Jobs is the address of a Device_Frame_Jobs' first element,
	-- Flags are Frames_Linked / Frames_Exact (1, 2), Dict may be null (the
	-- call is then the one without a dictionary), the result is the status
	-- of the call (0, or 5: Too_Little_Memory with Out_Len the bound, or 6:
	-- misuse).  A job with Status 9 and Reason 8 (LZ4ADA_DEVFRAME_DICT)
	-- names another dictionary id than Dict_Id (compared only with
	-- Dict_Check_Id in Flags).  For a frame answered with Status 9,
	-- Decode_Frame_Dict_Host decodes its host bytes against the dictionary's
	-- host bytes: plain host code, statuses 1, 2, 3 and 5 as the exceptions
	-- of LZ4Ada.
	Dict_Check_Id: constant Interfaces.Unsigned_32 := 1;
	type Device_Dict is record
		D_Dict:   System.Address;
		Dict_Len: Interfaces.Integer_64;
		Dict_Id:  Interfaces.Unsigned_32;
		Flags:    Interfaces.Unsigned_32;
	end record;
	pragma Convention(C, Device_Dict);
	function Frames_Device_Bound_Dict(D_In: System.Address; In_Len: Interfaces.Integer_64;
			Jobs: System.Address; N_Jobs: Interfaces.Integer_64;
			Flags: Interfaces.Unsigned_32; Dict: access constant Device_Dict;
			Bound: access Interfaces.Integer_64; Stream: System.Address)
			return Interfaces.Integer_32;
	pragma Import(C, Frames_Device_Bound_Dict, "lz4ada_frames_device_bound_dict");
	function Decode_Frames_Device_Dict(D_In: System.Address; In_Len: Interfaces.Integer_64;
			Jobs: System.Address; N_Jobs: Interfaces.Integer_64;
			Flags: Interfaces.Unsigned_32; Dict: access constant Device_Dict;
			D_Out: System.Address; Out_Cap: Interfaces.Integer_64;
			Out_Len: access Interfaces.Integer_64; Stream: System.Address)
			return Interfaces.Integer_32;
	pragma Import(C, Decode_Frames_Device_Dict, "lz4ada_decode_frames_device_dict");
	function Decode_Frame_Dict_Host(Frame: System.Address; Len: Interfaces.Integer_64;
			Dict: System.Address; Dict_Len: Interfaces.Integer_64;
			Out_Buf: System.Address; Out_Cap: Interfaces.Integer_64;
			Out_Len, Consumed: access Interfaces.Integer_64)
			return Interfaces.Integer_32;
	pragma Import(C, Decode_Frame_Dict_Host, "lz4ada_decode_frame_dict_host");

	-- lz4ada_compress_frames_device_indexed: records that lie in device
	-- memory compressed into LZ4 frames there, with the frames' seek index
	-- written by the same call (lz4ada_compress_index_options of
	-- include/lz4ada_hip.h; no reference twin).  The thin import, in the
	-- style of the dictionary calls above: Jobs is the address of the first
	-- of N_Jobs lz4ada_compress_job records, Opt that of an
	-- lz4ada_compress_options (null: 64 KiB blocks, no flag), Dict may be
	-- null, X_Opt may be null (frames of independent blocks), Frames is null
	-- or the address of a Device_Frame_Jobs' first element, Idx receives the
	-- index (an lz4ada_seek_index, to be handed to the ranged decode and
	-- freed with lz4ada_seek_index_free).  The result is the status of the
	-- call (0, or 5: Too_Little_Memory with Out_Len the bound, or 6: misuse;
	-- Idx is then null).
	Comp_Index_Linked: constant Interfaces.Unsigned_32 := 1;
	type Compress_Index_Options is record
		Flags:            Interfaces.Unsigned_32;
		Reserved:         Interfaces.Unsigned_32 := 0;
		Checkpoint_Bytes: Interfaces.Integer_64 := 0;
	end record;
	pragma Convention(C, Compress_Index_Options);
	function Compress_Frames_Device_Indexed(D_In: System.Address; In_Len: Interfaces.Integer_64;
			Jobs: System.Address; N_Jobs: Interfaces.Integer_64;
			Opt: System.Address; Dict: System.Address;
			X_Opt: access constant Compress_Index_Options;
			D_Out: System.Address; Out_Cap: Interfaces.Integer_64;
			Out_Len: access Interfaces.Integer_64; Frames: System.Address;
			Idx: access System.Address; Stream: System.Address)
			return Interfaces.Integer_32;
	pragma Import(C, Compress_Frames_Device_Indexed, "lz4ada_compress_frames_device_indexed");

	-- lz4ada_rccl_version: the RCCL this process bound (22606 = 2.26.6).
	function RCCL_Version return Interfaces.Integer_32;
	pragma Import(C, RCCL_Version, "lz4ada_rccl_version");

private

	function C_Decode_Frame(Frame: System.Address; Len: Interfaces.Integer_64;
			Out_Buf: System.Address; Out_Cap: Interfaces.Integer_64;
			Out_Len, Consumed: access Interfaces.Integer_64)
			return Interfaces.Integer_32;
	pragma Import(C, C_Decode_Frame, "lz4ada_decode_frame");

	function C_Decode_Stream(Input: System.Address; Len: Interfaces.Integer_64;
			Out_Buf: System.Address; Out_Cap: Interfaces.Integer_64;
			Out_Len: access Interfaces.Integer_64)
			return Interfaces.Integer_32;
	pragma Import(C, C_Decode_Stream, "lz4ada_decode_stream");

	function C_Decoded_Bound(Input: System.Address; Len: Interfaces.Integer_64)
			return Interfaces.Integer_64;
	pragma Import(C, C_Decoded_Bound, "lz4ada_decoded_bound");

	function C_Decode_Frame_Multi(Frame: System.Address; Len: Interfaces.Integer_64;
			N_GPUs: Interfaces.Integer_32; Devices: System.Address;
			Out_Buf: System.Address; Out_Cap: Interfaces.Integer_64;
			Out_Len, Consumed: access Interfaces.Integer_64)
			return Interfaces.Integer_32;
	pragma Import(C, C_Decode_Frame_Multi, "lz4ada_decode_frame_multi");

	function C_Decode_Frames(Jobs: System.Address; N_Jobs: Interfaces.Integer_64;
			Out_Buf: access System.Address;
			Out_Len: access Interfaces.Integer_64)
			return Interfaces.Integer_32;
	pragma Import(C, C_Decode_Frames, "lz4ada_decode_frames");

	function C_Frames_Device_Bound(D_In: System.Address; In_Len: Interfaces.Integer_64;
			Jobs: System.Address; N_Jobs: Interfaces.Integer_64;
			Bound: access Interfaces.Integer_64; Stream: System.Address)
			return Interfaces.Integer_32;
	pragma Import(C, C_Frames_Device_Bound, "lz4ada_frames_device_bound");

	function C_Decode_Frames_Device(D_In: System.Address; In_Len: Interfaces.Integer_64;
			Jobs: System.Address; N_Jobs: Interfaces.Integer_64;
			D_Out: System.Address; Out_Cap: Interfaces.Integer_64;
			Out_Len: access Interfaces.Integer_64; Stream: System.Address)
			return Interfaces.Integer_32;
	pragma Import(C, C_Decode_Frames_Device, "lz4ada_decode_frames_device");

	-- the same three with flags (LZ4ADA_FRAMES_LINKED = 1, LZ4ADA_FRAMES_EXACT = 2)
	Frames_Linked: constant Interfaces.Unsigned_32 := 1;
	Frames_Exact:  constant Interfaces.Unsigned_32 := 2;

	function C_Decode_Frames_Opt(Jobs: System.Address; N_Jobs: Interfaces.Integer_64;
			Flags: Interfaces.Unsigned_32;
			Out_Buf: access System.Address;
			Out_Len: access Interfaces.Integer_64)
			return Interfaces.Integer_32;
	pragma Import(C, C_Decode_Frames_Opt, "lz4ada_decode_frames_opt");

	function C_Frames_Device_Bound_Opt(D_In: System.Address; In_Len: Interfaces.Integer_64;
			Jobs: System.Address; N_Jobs: Interfaces.Integer_64;
			Flags: Interfaces.Unsigned_32;
			Bound: access Interfaces.Integer_64; Stream: System.Address)
			return Interfaces.Integer_32;
	pragma Import(C, C_Frames_Device_Bound_Opt, "lz4ada_frames_device_bound_opt");

	function C_Decode_Frames_Device_Opt(D_In: System.Address; In_Len: Interfaces.Integer_64;
			Jobs: System.Address; N_Jobs: Interfaces.Integer_64;
			Flags: Interfaces.Unsigned_32;
			D_Out: System.Address; Out_Cap: Interfaces.Integer_64;
			Out_Len: access Interfaces.Integer_64; Stream: System.Address)
			return Interfaces.Integer_32;
	pragma Import(C, C_Decode_Frames_Device_Opt, "lz4ada_decode_frames_device_opt");

	function C_Frames_Device_Sizes(D_In: System.Address; In_Len: Interfaces.Integer_64;
			Jobs: System.Address; N_Jobs: Interfaces.Integer_64;
			Flags: Interfaces.Unsigned_32;
			Total: access Interfaces.Integer_64; Stream: System.Address)
			return Interfaces.Integer_32;
	pragma Import(C, C_Frames_Device_Sizes, "lz4ada_frames_device_sizes");

end LZ4Ada.GPU;
