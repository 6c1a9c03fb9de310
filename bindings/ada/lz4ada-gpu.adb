-- lz4ada-gpu.adb -- UNTESTED (no GNAT in this image).
with Interfaces.C.Strings;

package body LZ4Ada.GPU is

	use type Interfaces.Integer_32;

	function C_Thread_Last_Error return Interfaces.C.Strings.chars_ptr;
	pragma Import(C, C_Thread_Last_Error, "lz4ada_thread_last_error");

	procedure Check(Status: Interfaces.Integer_32) is
		Text: constant String :=
			Interfaces.C.Strings.Value(C_Thread_Last_Error);
	begin
		case Status is
		when 0 => null;
		when 1 => raise Checksum_Error with Text;
		when 2 => raise Data_Corruption with Text;
		when 3 => raise Not_Supported with Text;
		when 4 => raise Too_Few_Header_Bytes with Text;
		when 5 => raise Too_Little_Memory with Text;
		when 6 => raise Program_Error with Text;
		when 7 => raise Constraint_Error with Text;
		when others => raise Device_Error with Text;
		end case;
	end Check;

	procedure Decode_Frame(Frame:          in     Octets;
				Output:         in out Octets;
				Output_Length:  out    Interfaces.Integer_64;
				Frame_Consumed: out    Interfaces.Integer_64) is
		L, C: aliased Interfaces.Integer_64;
	begin
		Check(C_Decode_Frame(Frame'Address, Frame'Length,
			Output'Address, Output'Length, L'Access, C'Access));
		Output_Length  := L;
		Frame_Consumed := C;
	end Decode_Frame;

	procedure Decode_Stream(Input:         in     Octets;
				Output:        in out Octets;
				Output_Length: out    Interfaces.Integer_64) is
		L: aliased Interfaces.Integer_64;
	begin
		Check(C_Decode_Stream(Input'Address, Input'Length,
			Output'Address, Output'Length, L'Access));
		Output_Length := L;
	end Decode_Stream;

	function Decoded_Bound(Input: in Octets) return Interfaces.Integer_64 is
	begin
		return C_Decoded_Bound(Input'Address, Input'Length);
	end Decoded_Bound;

	procedure Decode_Frame_Multi(Frame:          in     Octets;
				N_GPUs:         in     Positive;
				Output:         in out Octets;
				Output_Length:  out    Interfaces.Integer_64;
				Frame_Consumed: out    Interfaces.Integer_64) is
		L, C: aliased Interfaces.Integer_64;
	begin
		Check(C_Decode_Frame_Multi(Frame'Address, Frame'Length,
			Interfaces.Integer_32(N_GPUs), System.Null_Address,
			Output'Address, Output'Length, L'Access, C'Access));
		Output_Length  := L;
		Frame_Consumed := C;
	end Decode_Frame_Multi;

	procedure Decode_Frames(Jobs:          in out Frame_Jobs;
				Output:        out    System.Address;
				Output_Length: out    Interfaces.Integer_64;
				Linked:        in     Boolean := False) is
		P: aliased System.Address;
		L: aliased Interfaces.Integer_64;
	begin
		if Linked then
			Check(C_Decode_Frames_Opt(Jobs'Address, Jobs'Length, Frames_Linked,
				P'Access, L'Access));
		else
			Check(C_Decode_Frames(Jobs'Address, Jobs'Length, P'Access, L'Access));
		end if;
		Output        := P;
		Output_Length := L;
	end Decode_Frames;

	function Frames_Device_Bound(D_In:   in     System.Address;
				In_Len: in     Interfaces.Integer_64;
				Jobs:   in out Device_Frame_Jobs;
				Stream: in     System.Address := System.Null_Address;
				Linked: in     Boolean := False)
				return Interfaces.Integer_64 is
		B: aliased Interfaces.Integer_64;
	begin
		if Linked then
			Check(C_Frames_Device_Bound_Opt(D_In, In_Len, Jobs'Address, Jobs'Length,
				Frames_Linked, B'Access, Stream));
		else
			Check(C_Frames_Device_Bound(D_In, In_Len, Jobs'Address, Jobs'Length,
				B'Access, Stream));
		end if;
		return B;
	end Frames_Device_Bound;

	function Frames_Device_Sizes(D_In:   in     System.Address;
				In_Len: in     Interfaces.Integer_64;
				Jobs:   in out Device_Frame_Jobs;
				Stream: in     System.Address := System.Null_Address;
				Linked: in     Boolean := False)
				return Interfaces.Integer_64 is
		T: aliased Interfaces.Integer_64;
	begin
		Check(C_Frames_Device_Sizes(D_In, In_Len, Jobs'Address, Jobs'Length,
			(if Linked then Frames_Linked else 0), T'Access, Stream));
		return T;
	end Frames_Device_Sizes;

	procedure Decode_Frames_Device(D_In:          in     System.Address;
				In_Len:        in     Interfaces.Integer_64;
				Jobs:          in out Device_Frame_Jobs;
				D_Out:         in     System.Address;
				Out_Cap:       in     Interfaces.Integer_64;
				Output_Length: out    Interfaces.Integer_64;
				Stream:        in     System.Address := System.Null_Address;
				Linked:        in     Boolean := False;
				Exact:         in     Boolean := False) is
		use type Interfaces.Unsigned_32;
		L:  aliased Interfaces.Integer_64;
		St: Interfaces.Integer_32;
	begin
		if Linked or Exact then
			St := C_Decode_Frames_Device_Opt(D_In, In_Len, Jobs'Address, Jobs'Length,
				(if Linked then Frames_Linked else 0) or (if Exact then Frames_Exact else 0),
				D_Out, Out_Cap, L'Access, Stream);
		else
			St := C_Decode_Frames_Device(D_In, In_Len, Jobs'Address, Jobs'Length,
				D_Out, Out_Cap, L'Access, Stream);
		end if;
		Output_Length := L;  -- the bound, when Too_Little_Memory follows
		Check(St);
	end Decode_Frames_Device;

	function Frames_Error(Jobs: in Frame_Jobs; I: in Positive) return String is
		function C_Frames_Error(J: Interfaces.Integer_64)
				return Interfaces.C.Strings.chars_ptr;
		pragma Import(C, C_Frames_Error, "lz4ada_frames_error");
	begin
		return Interfaces.C.Strings.Value(C_Frames_Error(
				Interfaces.Integer_64(I - Jobs'First)));
	end Frames_Error;

end LZ4Ada.GPU;
